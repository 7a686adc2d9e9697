#!/usr/bin/env python3
"""The grouped 3x3 conv kernels (csrc/conv_group.hip) next to the path ResNeXt took before them.

* ``kernels``: ``K.group_conv_fwd`` / ``group_conv_dgrad`` / ``group_conv_wgrad`` at the conv2 shapes of
  ``resnext50_32x4d`` (batch 256) against ``torch.nn.functional.conv2d(groups=)`` on channels_last bf16 tensors
  (forward; backward as ``torch.autograd.grad`` for the input and for the weight). Each in a captured graph of
  ``--launches`` launches, alternated native, torch, native per round; the spread of the two native readings of a
  round is the yardstick. Beside each reading: the bytes the operation must move (every operand and result once)
  over the probed streaming roof, and the native time as a multiple of it.
* ``steps``: ``NativeTrainer`` against ``AutogradTrainer`` on one model and one resident batch, alternated.
  python tools/bench_gconv.py [--models resnext50_32x4d:224:128,wide_resnet50_2:224:128] [--rounds 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dbx_distributed_pytorch_examples_amd.engine.autograd_trainer import AutogradTrainer  # noqa: E402
from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig  # noqa: E402
from dbx_distributed_pytorch_examples_amd.models import build_model  # noqa: E402
from dbx_distributed_pytorch_examples_amd.ops import kernels as K  # noqa: E402

ROOF_TBS = 5.9  # mixed read/write streaming roof (the lower probe of profiles/r6_roof/)
# resnext50_32x4d conv2 at 224: (H = W of the input, C, stride), groups = 32
SHAPES = ((56, 128, 1), (56, 256, 2), (28, 256, 1), (28, 512, 2), (14, 512, 1), (14, 1024, 2), (7, 1024, 1))


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out is not None:
        out.write(line + "\n")
        out.flush()


def graph_of(fn, launches, dev):
    fn()
    torch.cuda.synchronize(dev)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(launches):
            fn()
    gr.replay()
    torch.cuda.synchronize(dev)
    return gr


def window(gr, launches, dev, seconds=0.3):
    reps, dt = 2, 0.0
    while True:
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(reps):
            gr.replay()
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / (reps * launches)
        reps *= 2


def bench_kernels(N, H, Cc, stride, groups, rounds, launches, out):
    dev = torch.device("cuda", 0)
    cpg = Cc // groups
    OH, _ = K.conv_out_hw(H, H, 3, 3, stride, 1)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(N, H, H, Cc, generator=g).bfloat16().to(dev)
    dy = torch.randn(N, OH, OH, Cc, generator=g).bfloat16().to(dev)
    w = (torch.randn(Cc, 9 * cpg, generator=g) / (9 * cpg) ** 0.5).bfloat16().to(dev)
    y, dx = torch.empty_like(dy), torch.empty_like(x)
    dw = torch.empty(Cc, 9 * cpg, device=dev)
    ws = torch.empty(64 << 20, device=dev)
    stats = K.new_stats(Cc, dev)
    # torch: NCHW-shaped views of the same NHWC memory (channels_last)
    xt, dyt = x.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2)
    wt = w.view(Cc, 3, 3, cpg).permute(0, 3, 1, 2)
    xr, wr = xt.detach().requires_grad_(), wt.detach().requires_grad_()
    conv = lambda a, b: F.conv2d(a, b, stride=stride, padding=1, groups=groups)  # noqa: E731
    xb, wb, nb = x.numel() * 2, w.numel() * 2, dy.numel() * 2
    ops = {
        "fwd": (lambda: K.group_conv_fwd(x, w, y, groups=groups, stride=stride, stats=stats), lambda: conv(xt, wt),
                xb + wb + nb),
        "dgrad": (lambda: K.group_conv_dgrad(dy, w, dx, groups=groups, stride=stride),
                  lambda: torch.autograd.grad(conv(xr, wt), xr, dyt), nb + wb + xb),
        "wgrad": (lambda: K.group_conv_wgrad(dy, x, dw, ws, groups=groups, stride=stride),
                  lambda: torch.autograd.grad(conv(xt, wr), wr, dyt), nb + xb + 2 * wb),
    }
    for op, (native, ref, nbytes) in ops.items():
        # (torch's backward entries also run the forward they differentiate: its cost is reported apart and taken off)
        graphs = {"native": graph_of(native, launches, dev), "torch": graph_of(ref, launches, dev)}
        fwd_us = 0.0
        if op != "fwd":
            fwd_us = 1e6 * window(graph_of(lambda: conv(xt, wt), launches, dev), launches, dev)
        roof_us = nbytes / (ROOF_TBS * 1e12) * 1e6
        reads = {"native": [], "torch": []}
        for r in range(rounds):
            for slot, name in enumerate(("native", "torch", "native")):
                us = 1e6 * window(graphs[name], launches, dev) - (fwd_us if name == "torch" else 0.0)
                reads[name].append(us)
                emit({"op": op, "path": name, "N": N, "H": H, "C": Cc, "groups": groups, "stride": stride, "round": r,
                      "slot": slot, "us": us}, out)
        nat, tor = reads["native"], reads["torch"]
        m_nat, m_tor = sum(nat) / len(nat), sum(tor) / len(tor)
        emit({"summary": "kernel", "op": op, "N": N, "H": H, "C": Cc, "cpg": cpg, "stride": stride, "bytes": nbytes,
              "roof_us": roof_us, "native_us": m_nat, "torch_us": m_tor, "torch_fwd_us_taken_off": fwd_us,
              "native_spread_us": max(nat) - min(nat), "native_over_roof": m_nat / roof_us,
              "torch_over_native": m_tor / m_nat}, out)


def bench_model(arch, hw, batch, rounds, seconds, out):
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (batch, hw, hw, 3), dtype=torch.uint8, generator=g).to(dev)
    lab = torch.randint(0, 1000, (batch,), generator=g).to(dev)
    torch.manual_seed(0)
    nat = NativeTrainer(build_model(arch), batch, (hw, hw), dev, optim=OptimConfig(lr=1e-3))
    nat.step(img, lab)
    for _ in range(3):
        nat.step()
    ref = AutogradTrainer(build_model(arch).to(dev), dev, OptimConfig(lr=1e-3))
    xf = nat.prog.x4[..., :3].permute(0, 3, 1, 2).float().contiguous(memory_format=torch.channels_last)
    steps = {"native": nat.step, "autograd": lambda: ref.step(xf, lab)}
    for _ in range(3):
        steps["autograd"]()
    torch.cuda.synchronize(dev)

    def run(name, n):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(n):
            steps[name]()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / n

    reads = {"native": [], "autograd": []}
    for r in range(rounds):
        for slot, name in enumerate(("native", "autograd", "native")):
            per = run(name, 4)
            ms = 1e3 * run(name, max(4, int(seconds / per)))
            reads[name].append(ms)
            emit({"model": arch, "hw": hw, "batch": batch, "engine": name, "round": r, "slot": slot, "ms_per_step": ms,
                  "img_per_s": batch / ms * 1e3}, out)
    m = {k: sum(v) / len(v) for k, v in reads.items()}
    emit({"summary": "steps", "model": arch, "hw": hw, "batch": batch, "native_ms": m["native"],
          "autograd_ms": m["autograd"], "native_spread_ms": max(reads["native"]) - min(reads["native"]),
          "native_img_per_s": batch / m["native"] * 1e3, "autograd_img_per_s": batch / m["autograd"] * 1e3,
          "autograd_over_native": m["autograd"] / m["native"]}, out)
    del nat, ref, steps
    import gc
    gc.collect()
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--models", default="resnext50_32x4d:224:128,wide_resnet50_2:224:128",
                   help="arch:image size:batch, ... ('' = none)")
    p.add_argument("--batch", type=int, default=256, help="batch of the kernel shapes")
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--seconds", type=float, default=1.0, help="least duration of one step reading")
    p.add_argument("--launches", type=int, default=20, help="kernel launches per captured graph")
    p.add_argument("--no-kernels", action="store_true")
    p.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = p.parse_args()
    if not torch.cuda.is_available():
        print("bench_gconv: no GPU (a timing needs the device)", file=sys.stderr)
        sys.exit(2)
    out = open(a.out, "a") if a.out else None
    if not a.no_kernels:
        for H, Cc, stride in SHAPES:
            bench_kernels(a.batch, H, Cc, stride, 32, a.rounds, a.launches, out)
    for spec in filter(None, a.models.split(",")):
        arch, hw, batch = spec.split(":")
        bench_model(arch, int(hw), int(batch), a.rounds, a.seconds, out)
    if out is not None:
        out.close()


if __name__ == "__main__":
    main()
