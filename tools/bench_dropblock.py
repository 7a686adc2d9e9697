#!/usr/bin/env python3
"""The DropBlock kernels (csrc/dropblock_ops.hip) beside the bytes they must move, and a resnet50 step with and without
DropBlock beside the autograd engine.

* ``kernels``: ``K.dropblock_mask``, ``K.dropblock_fwd``, ``K.dropblock_bn_bwd_reduce`` and ``K.dropblock_bn_bwd_apply``
  at the two kinds of site of ``resnet50`` at 224 (batch 256), each in a captured graph of ``--launches`` launches.
  Beside each reading: the bytes the kernel must move (every tensor once; the mask kernel: the bit it writes per
  element) over the streaming roof and the time as a multiple of it; for the mask kernel also its Philox calls per
  second (one per four elements of the valid interior).
* ``steps``: ``NativeTrainer`` with ``drop_block_rate`` 0.1 and 0, and ``AutogradTrainer`` with 0.1, on one resident
  batch, alternated in one process.
  python tools/bench_dropblock.py [--step resnet50:224:128] [--rounds 3] [--out FILE]
The default workload against the parent commit is ``bench.py`` itself, run from both trees in alternation.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_gconv import ROOF_TBS, emit, graph_of, window  # noqa: E402
from dbx_distributed_pytorch_examples_amd.engine.autograd_trainer import AutogradTrainer  # noqa: E402
from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig  # noqa: E402
from dbx_distributed_pytorch_examples_amd.models import build_model  # noqa: E402
from dbx_distributed_pytorch_examples_amd.ops import kernels as K  # noqa: E402

# resnet50 at 224: (H = W, C of bn2, block size, gamma scale) in layer3 and layer4
SITES = ((14, 256, 5, 0.25), (7, 512, 3, 1.0))


def bench_kernels(N, H, Cc, bs, gs, p, rounds, launches, out):
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(H * 1000 + Cc)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    bf = torch.bfloat16
    y, das = rn(N, H, H, Cc).to(bf), rn(N, H, H, Cc).to(bf)
    full = torch.empty_like(y)
    gamma, beta, mean, invstd = 1 + 0.1 * rn(Cc), 0.1 * rn(Cc), 0.1 * rn(Cc), 1 + 0.1 * rn(Cc).abs()
    sc, sh = gamma * invstd, beta - gamma * invstd * mean
    bst, coeff = K.new_stats(Cc, dev, nshard=4), torch.zeros(3 * Cc, device=dev)
    bits = torch.empty(N, H, H, Cc // 32, device=dev, dtype=torch.int32)
    kept, off = torch.zeros(1, device=dev, dtype=torch.int64), torch.ones(1, device=dev, dtype=torch.int32)
    bs_eff, gam = K.dropblock_geometry(H, H, bs, p, gs)
    thr = torch.tensor([K.dropblock_threshold(gam)], dtype=torch.int32, device=dev)
    K.dropblock_mask(bits, kept, thr, off, block_size=bs, seed=1, site=0)  # kept: this one mask's count from here on
    b_act, b_bits = y.numel() * 2, bits.numel() * 4
    calls = N * (H - bs_eff + 1) ** 2 * Cc // 4
    scratch = torch.empty_like(bits)  # (the timed mask launches write here: kept stays the count of ``bits``)
    kscratch = torch.zeros(1, device=dev, dtype=torch.int64)
    ops = {  # name -> (launch, bytes it must move)
        "dropblock_mask": (lambda: K.dropblock_mask(scratch, kscratch, thr, off, block_size=bs, seed=1, site=0), b_bits),
        "dropblock_fwd": (lambda: K.dropblock_fwd(y, sc, sh, bits, kept, full), 2 * b_act + b_bits),
        "dropblock_bn_bwd_reduce": (lambda: K.dropblock_bn_bwd_reduce(das, y, sc, sh, bits, kept, mean, invstd, bst),
                                    2 * b_act + b_bits),
        "dropblock_bn_bwd_apply": (lambda: K.dropblock_bn_bwd_apply(das, y, sc, sh, bits, kept, coeff, full),
                                   3 * b_act + b_bits),
    }
    for fn, _ in ops.values():
        fn()
    K.bn_bwd_coeff(bst, N * H * H, gamma, mean, invstd, coeff)
    graphs = {k: graph_of(fn, launches, dev) for k, (fn, _) in ops.items()}
    for k, (_, nbytes) in ops.items():
        us = sorted(window(graphs[k], launches, dev) * 1e6 for _ in range(rounds))
        roof = nbytes / (ROOF_TBS * 1e12) * 1e6
        rec = dict(kind="kernel", op=k, N=N, H=H, C=Cc, block_size=bs, us_median=round(us[len(us) // 2], 2),
                   us_spread=round(us[-1] - us[0], 2), bytes=nbytes, roof_us=round(roof, 2),
                   x_roof=round(us[len(us) // 2] / roof, 2))
        if k == "dropblock_mask":
            rec["philox_calls"] = calls
            rec["philox_gcalls_per_s"] = round(calls / us[len(us) // 2] * 1e-3, 2)
        emit(rec, out)


def bench_steps(arch, hw, batch, rate, rounds, seconds, out):
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (batch, hw, hw, 3), dtype=torch.uint8, generator=g).to(dev)
    lab = torch.randint(0, 1000, (batch,), generator=g).to(dev)
    steps = {}
    for name, r in (("native_dropblock", rate), ("native_plain", 0.0)):
        torch.manual_seed(0)
        tr = NativeTrainer(build_model(arch, drop_block_rate=r), batch, (hw, hw), dev, optim=OptimConfig(lr=1e-3))
        tr.step(img, lab)
        for _ in range(3):
            tr.step()
        steps[name] = tr.step
    ref = AutogradTrainer(build_model(arch, drop_block_rate=rate).to(dev), dev, OptimConfig(lr=1e-3))
    xf = tr.prog.x4[..., :3].permute(0, 3, 1, 2).float().contiguous(memory_format=torch.channels_last)
    steps["autograd_dropblock"] = lambda: ref.step(xf, lab)
    for _ in range(3):
        steps["autograd_dropblock"]()

    def run(name, n):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(n):
            steps[name]()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / n

    for r in range(rounds):
        for slot, name in enumerate(("native_dropblock", "native_plain", "autograd_dropblock", "native_dropblock",
                                     "native_plain")):
            per = run(name, 4)
            ms = 1e3 * run(name, max(4, int(seconds / per)))
            emit({"kind": "step", "model": arch, "hw": hw, "batch": batch, "drop_block_rate": rate, "engine": name,
                  "round": r, "slot": slot, "ms_per_step": round(ms, 3), "img_per_s": round(batch / ms * 1e3, 1)}, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rate", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--step", default="", help="name:size:batch for the step comparison")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dropblock.py measures on a GPU; none is visible")
    out = open(a.out, "a") if a.out else None
    for H, Cc, bs, gs in SITES:
        bench_kernels(a.batch, H, Cc, bs, gs, a.rate, a.rounds, a.launches, out)
    if a.step:
        name, size, batch = a.step.split(":")
        bench_steps(name, int(size), int(batch), a.rate, a.rounds, 1.0, out)


if __name__ == "__main__":
    main()
