#!/usr/bin/env python3
"""The blur-pool kernels (csrc/blur_ops.hip) beside the bytes they must move, and resnetblur50 beside autograd.

* ``kernels``: ``K.blur_fwd`` (with the BN + ReLU prologue), ``K.blur_bwd``, ``K.blur_bn_bwd_reduce`` and
  ``K.blur_bn_bwd_apply`` at the four blur sites of ``resnetblur50`` at 224 (batch 256), each in a captured graph of
  ``--launches`` launches. Beside each reading: the bytes the kernel must move (every tensor once) over the streaming
  roof, and the time as a multiple of it.
* ``steps``: ``NativeTrainer`` against ``AutogradTrainer`` on one model and one resident batch, alternated.
  python tools/bench_blur.py [--models resnetblur50:224:128,resnet50:224:128] [--rounds 3] [--out FILE]
The default workload against the parent commit is ``bench.py`` itself, run from both trees in alternation.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_gconv import ROOF_TBS, bench_model, emit, graph_of, window  # noqa: E402
from dbx_distributed_pytorch_examples_amd.ops import kernels as K  # noqa: E402

# resnetblur50 at 224: (H = W before the blur, C) of the stem pool and of conv2 in layer2.0 / layer3.0 / layer4.0
SHAPES = ((112, 64), (56, 128), (28, 256), (14, 512))


def bench_kernels(N, H, Cc, rounds, launches, out):
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(H * 1000 + Cc)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    bf = torch.bfloat16
    P, Q = K.blur_out_hw(H, H)
    y, dpool = rn(N, H, H, Cc).to(bf), rn(N, P, Q, Cc).to(bf)
    small, full = torch.empty_like(dpool), torch.empty_like(y)
    gamma, beta, mean, invstd = 1 + 0.1 * rn(Cc), 0.1 * rn(Cc), 0.1 * rn(Cc), 1 + 0.1 * rn(Cc).abs()
    sc, sh = gamma * invstd, beta - gamma * invstd * mean
    bst, coeff = K.new_stats(Cc, dev, nshard=4), torch.zeros(3 * Cc, device=dev)
    b_full, b_small = y.numel() * 2, dpool.numel() * 2
    ops = {  # name -> (launch, bytes it must move)
        "blur_fwd": (lambda: K.blur_fwd(y, small, scale=sc, shift=sh), b_full + b_small),
        "blur_bwd": (lambda: K.blur_bwd(dpool, full), b_full + b_small),
        "blur_bn_bwd_reduce": (lambda: K.blur_bn_bwd_reduce(dpool, y, sc, sh, mean, invstd, bst), b_full + b_small),
        "blur_bn_bwd_apply": (lambda: K.blur_bn_bwd_apply(dpool, y, sc, sh, coeff, full), 2 * b_full + b_small),
    }
    for fn, _ in ops.values():
        fn()
    K.bn_bwd_coeff(bst, N * H * H, gamma, mean, invstd, coeff)
    graphs = {k: graph_of(fn, launches, dev) for k, (fn, _) in ops.items()}
    for k, (_, nbytes) in ops.items():
        us = sorted(window(graphs[k], launches, dev) * 1e6 for _ in range(rounds))
        roof = nbytes / (ROOF_TBS * 1e12) * 1e6
        emit(dict(kind="kernel", op=k, N=N, H=H, C=Cc, us_median=round(us[len(us) // 2], 2),
                  us_spread=round(us[-1] - us[0], 2), bytes=nbytes, roof_us=round(roof, 2),
                  x_roof=round(us[len(us) // 2] / roof, 2)), out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--models", default="", help="name:size:batch,... for the step comparison")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_blur.py measures on a GPU; none is visible")
    out = open(a.out, "a") if a.out else None
    for H, Cc in SHAPES:
        bench_kernels(a.batch, H, Cc, a.rounds, a.launches, out)
    for spec in filter(None, a.models.split(",")):
        name, size, batch = spec.split(":")
        bench_model(name, int(size), int(batch), a.rounds, 1.0, out)


if __name__ == "__main__":
    main()
