#!/usr/bin/env python3
"""The squeeze-and-excitation kernels (csrc/se_ops.hip) beside the bytes they must move and beside torch.

* ``kernels``: the six ``K.se_*`` kernels at the block-tail shapes of ``seresnet50`` (batch 256), each in a captured
  graph of ``--launches`` launches. Beside each reading: the bytes the kernel must move (the big tensors once; the
  per-sample tables and weights are counted too) over the streaming roof, and the time as a multiple of it. The
  forward trio is also timed as the same operation in torch on channels_last bf16 tensors.
* ``steps``: ``NativeTrainer`` against ``AutogradTrainer`` on one model and one resident batch, alternated.
  python tools/bench_se.py [--models seresnet50:224:128,resnet50:224:128] [--rounds 3] [--out FILE]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_gconv import ROOF_TBS, bench_model, emit, graph_of, window  # noqa: E402
from dbx_distributed_pytorch_examples_amd.ops import kernels as K  # noqa: E402

# seresnet50 block tails at 224: (H = W, C, rd)
SHAPES = ((56, 256, 16), (28, 512, 32), (14, 1024, 64), (7, 2048, 128))


def bench_kernels(N, H, Cc, rd, rounds, launches, out):
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(H * 1000 + Cc)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    bf, HW = torch.bfloat16, H * H
    y, gr_, res = rn(N, H, H, Cc).to(bf), rn(N, H, H, Cc).to(bf), rn(N, H, H, Cc).to(bf)
    out_, dy, gout = torch.empty_like(y), torch.empty_like(y), torch.empty_like(y)
    bits = torch.zeros(y.numel() // 8, device=dev, dtype=torch.uint8)
    gamma, beta, mean, invstd = 1 + 0.1 * rn(Cc), 0.1 * rn(Cc), 0.1 * rn(Cc), 1 + 0.1 * rn(Cc).abs()
    sc, sh = gamma * invstd, beta - gamma * invstd * mean
    w1, b1, w2, b2 = (rn(rd, Cc) / Cc ** 0.5).to(bf), 0.1 * rn(rd), (rn(Cc, rd) / rd ** 0.5).to(bf), 0.1 * rn(Cc)
    f32 = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    zsum, gate, A, B, dz, coeff = f32(N, Cc), f32(N, Cc), f32(N, Cc), f32(N, Cc), f32(N, Cc), f32(3 * Cc)
    zq, dpre2, h, dpre1 = f32(N, Cc).to(bf), f32(N, Cc).to(bf), f32(N, rd).to(bf), f32(N, rd).to(bf)
    bst = K.new_stats(Cc, dev, nshard=4)
    ws = torch.empty(K.se_nsplit(HW) * 2 * N * Cc, device=dev)
    big, tab, wts = y.numel() * 2, N * Cc * 4, 2 * rd * Cc * 2
    ops = {  # name -> (launch, bytes it must move)
        "se_squeeze": (lambda: K.se_squeeze(y, zsum, ws=ws), big + tab),
        "se_excite": (lambda: K.se_excite(zsum, sc, sh, HW, w1, b1, w2, b2, zq, h, gate), 2 * tab + tab // 2 + wts),
        "se_tail": (lambda: K.se_tail(y, sc, sh, gate, out_, res=res, mbits=bits), 3 * big + big // 16 + tab),
        "se_bwd_reduce": (lambda: K.se_bwd_reduce(gr_, bits, y, mean, invstd, A, B, ws=ws), 2 * big + big // 16 + 2 * tab),
        "se_excite_bwd": (lambda: K.se_excite_bwd(A, B, gate, h, zsum, HW, gamma, beta, mean, invstd, w2, w1, dpre2,
                                                  dpre1, dz, bst), 2 * (5 * tab) + tab // 2 + wts),
        "se_bwd_apply": (lambda: K.se_bwd_apply(gr_, bits, y, gate, dz, coeff, dy, gout), 4 * big + big // 16 + 2 * tab),
    }
    for fn, _ in ops.values():  # (in order: each fills what the next reads)
        fn()
    K.bn_bwd_coeff(bst, N * HW, gamma, mean, invstd, coeff)
    yc = y.permute(0, 3, 1, 2)  # channels_last views of the same memory
    rc, w1f, w2f = res.permute(0, 3, 1, 2), w1.view(rd, Cc, 1, 1), w2.view(Cc, rd, 1, 1)

    def torch_fwd():
        u = yc * sc.to(bf).view(1, -1, 1, 1) + sh.to(bf).view(1, -1, 1, 1)
        s = torch.sigmoid(torch.conv2d(torch.relu(torch.conv2d(u.mean((2, 3), keepdim=True), w1f, b1.to(bf))), w2f,
                                       b2.to(bf)))
        return torch.relu(u * s + rc)
    ops["torch_forward"] = (torch_fwd, 4 * big)  # (the bytes of squeeze + tail)
    graphs = {k: graph_of(fn, launches, dev) for k, (fn, _) in ops.items()}
    for k, (_, nbytes) in ops.items():
        us = sorted(window(graphs[k], launches, dev) * 1e6 for _ in range(rounds))
        roof = nbytes / (ROOF_TBS * 1e12) * 1e6
        emit(dict(kind="kernel", op=k, N=N, H=H, C=Cc, rd=rd, us_median=round(us[len(us) // 2], 2),
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
        raise SystemExit("bench_se.py measures on a GPU; none is visible")
    out = open(a.out, "a") if a.out else None
    for H, Cc, rd in SHAPES:
        bench_kernels(a.batch, H, Cc, rd, a.rounds, a.launches, out)
    for spec in filter(None, a.models.split(",")):
        name, size, batch = spec.split(":")
        bench_model(name, int(size), int(batch), a.rounds, 1.0, out)


if __name__ == "__main__":
    main()
