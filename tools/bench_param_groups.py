#!/usr/bin/env python3
"""Cost of parameter groups in the native step, and of the grouped optimizer kernels alone.

Step: three NativeTrainers per model on synthetic resident data in one process -- two plain ones and one
with ``norm_weight_decay=0, bias_weight_decay=0`` (a dozen runs of the flat master) -- alternated per round
as (plain A, grouped, plain B): the spread between the two plain readings of a round is the yardstick for
grouped - plain. The grouped kernels move the same bytes as the plain ones (the run table is 12 KiB at
most, read once per block into LDS), so the bytes predict zero.

Kernels alone (``--kernels``): ``K.sgd_step`` / ``K.adam_step`` over the ResNet-50 flat size, plain against
grouped with (a) the dozen-run table of the two shorthands and (b) one run per tensor, timed with device
events over batches of launches, alternated (plain, grouped, plain) in one process.

One JSON line per reading and one summary line per comparison.
  python tools/bench_param_groups.py [--models resnet18:32:256,resnet50:224:1024] [--rounds 3] [--kernels] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig  # noqa: E402
from dbx_distributed_pytorch_examples_amd.models import build_model  # noqa: E402
from dbx_distributed_pytorch_examples_amd.ops import kernels as K  # noqa: E402


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out is not None:
        out.write(line + "\n")
        out.flush()


def summary(kind, key, readings, rounds, extra, out):
    a, g, b = readings["plain_a"], readings["grouped"], readings["plain_b"]
    plain = a + b
    m_plain, m_g = sum(plain) / len(plain), sum(g) / len(g)
    emit({kind: key, "summary": True, **extra, "plain_us": m_plain, "grouped_us": m_g,
          "plain_spread_within_round_us": max(abs(x - y) for x, y in zip(a, b)),
          "plain_spread_all_us": max(plain) - min(plain), "grouped_minus_plain_us": m_g - m_plain,
          "grouped_minus_plain_us_per_round": [g[r] - 0.5 * (a[r] + b[r]) for r in range(rounds)],
          "grouped_vs_plain": m_plain / m_g - 1.0}, out)


def bench_model(arch, hw, batch, optim, rounds, seconds, out):
    dev = torch.device("cuda", 0)
    classes = 1000 if hw >= 64 else 10
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (batch, hw, hw, 3), dtype=torch.uint8, generator=g).to(dev)
    lab = torch.randint(0, classes, (batch,), generator=g).to(dev)
    trs = {}
    for name in ("plain_a", "grouped", "plain_b"):
        torch.manual_seed(0)
        kw = dict(norm_weight_decay=0.0, bias_weight_decay=0.0) if name == "grouped" else {}
        o = OptimConfig(name=optim, lr=0.05 if optim == "sgd" else 1e-3, weight_decay=5e-5, **kw)
        trs[name] = NativeTrainer(build_model(arch, num_classes=classes), batch, (hw, hw), dev, optim=o)
        trs[name].step(img, lab)  # the resident batch; later steps reuse the static input buffers
        for _ in range(3):  # two eager warm-up steps in all, the capture, a replay
            trs[name].step()
        assert len(trs[name].graphs) == 1
    assert trs["grouped"].group_runs is not None and trs["plain_a"].group_runs is None
    nruns = len(trs["grouped"].group_runs._dbx_runs[2])
    torch.cuda.synchronize(dev)

    def window(name, n):
        tr = trs[name]
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(n):
            tr.step()
        torch.cuda.synchronize(dev)  # (the host clock ends behind the last kernel)
        return time.perf_counter() - t0

    per = window("plain_a", 8) / 8
    n = max(8, int(seconds / per + 7) // 8 * 8)
    readings = {k: [] for k in trs}
    for r in range(rounds):
        for slot, name in enumerate(("plain_a", "grouped", "plain_b")):
            dt = window(name, n)
            rec = {"model": arch, "hw": hw, "batch": batch, "optim": optim, "trainer": name, "round": r, "slot": slot,
                   "steps": n, "us_per_step": 1e6 * dt / n, "img_per_s": batch * n / dt}
            readings[name].append(rec["us_per_step"])
            emit(rec, out)
    summary("model", arch, readings, rounds,
            {"hw": hw, "batch": batch, "optim": optim, "n_params": trs["grouped"].prog.n_params, "runs": nruns,
             "updates_inside_backward": trs["grouped"].opt_ranges is not None}, out)
    tables = None
    if arch == "resnet50":
        tr = trs["grouped"]
        per_tensor = [(off, 5e-5 if i % 2 else 0.0, 1.0 if i % 4 else 0.5)
                      for i, (_, off, _) in enumerate(sorted(tr.prog.param_ranges, key=lambda r: r[1]))]
        tables = (tr.prog.n_params, {"dozen": tr.group_runs, "per_tensor": K.pack_opt_runs(per_tensor, tr.prog.n_params, dev)})
    trs.clear()
    import gc
    gc.collect()
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()
    return tables


def bench_kernels(n, tables, rounds, launches, out):
    """Plain against grouped launches over n elements (the ResNet-50 flat master), device-event timed."""
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    p, gr, m, v = (torch.randn(n, device=dev, generator=g) * 0.01 for _ in range(4))
    v.abs_()
    hyper = torch.tensor([1e-3, 0.1, 0.001], device=dev)

    def call(kind, tab):
        wd = dict(weight_decay=0.0, runs=tab, run_base=0) if tab is not None else dict(weight_decay=5e-5)
        o = OptimConfig(name="sgd" if kind == "sgd" else "adamw", lr=1e-3)  # momentum 0.9, betas (0.9, 0.999), eps 1e-8
        K.optim_step(o, p, gr, m, v, None, hyper=hyper, **wd)

    def window(kind, tab):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            call(kind, tab)
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / launches  # us per launch

    for kind in ("sgd", "adam"):
        for tname, tab in tables.items():
            for t in (None, tab):
                window(kind, t)  # warm-up
            readings = {"plain_a": [], "grouped": [], "plain_b": []}
            for r in range(rounds):
                for slot, (name, t) in enumerate((("plain_a", None), ("grouped", tab), ("plain_b", None))):
                    us = window(kind, t)
                    readings[name].append(us)
                    emit({"kernel": kind, "table": tname, "which": name, "round": r, "slot": slot, "n": n,
                          "launches": launches, "us_per_launch": us}, out)
            bytes_per = 20.0 if kind == "sgd" else 28.0  # r p, g, v; w p, v | r p, g, m, v; w p, m, v
            summary("kernel", kind, readings, rounds,
                    {"table": tname, "runs": (tab.numel() - 1) // 3, "n": n, "bytes_per_element": bytes_per}, out)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--models", default="resnet18:32:256,resnet50:224:1024", help="arch:image size:batch, ...")
    p.add_argument("--optim", default="sgd", choices=["sgd", "adamw"])
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--seconds", type=float, default=1.0, help="least duration of one step reading")
    p.add_argument("--kernels", action="store_true", help="also time the grouped kernels alone (needs resnet50 in --models)")
    p.add_argument("--launches", type=int, default=200, help="launches per kernel reading")
    p.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = p.parse_args()
    if not torch.cuda.is_available():
        print("bench_param_groups: no GPU (a timing needs the device)", file=sys.stderr)
        sys.exit(2)
    out = open(a.out, "a") if a.out else None
    tables = None
    for spec in a.models.split(","):
        arch, hw, batch = spec.split(":")
        t = bench_model(arch, int(hw), int(batch), a.optim, a.rounds, a.seconds, out)
        tables = t or tables
    if a.kernels:
        if tables is None:
            print("bench_param_groups: --kernels needs resnet50 among --models (its flat layout)", file=sys.stderr)
            sys.exit(2)
        bench_kernels(tables[0], tables[1], a.rounds, a.launches, out)
    if out is not None:
        out.close()


if __name__ == "__main__":
    main()
