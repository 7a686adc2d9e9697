#!/usr/bin/env python3
"""Cost of TrivialAugmentWide in the native step, one JSON line per record.

* ``"kernel"`` records: ``crop_resize_u8``, ``ta_prepare``, ``ta_apply_u8`` alone and the composed call (with its
  histogram memset), beside the plain and the mixing input kernel, per shape -- device events around
  ``--launches`` launches, plain / variant / plain per round (the two plain readings of a round are the spread).
  The table is drawn by the trainer's sampler, so the fourteen operations occur as they do in training. With
  the bytes each launch has to move (source, T written and read, output) and the rate that is of the time.
* ``"step"`` records: two NativeTrainers per model on synthetic resident data in one process, alternated (off, on,
  off per round: plain against plain is the yardstick for on - off), and a summary with the measured on - off
  beside the prediction from bytes: T is written once and read once, 4 bytes per pixel each way.

  python tools/bench_ta.py [--models resnet50:224:1024,resnet18:32:256] [--rounds 3] [--out FILE]
"""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dbx_distributed_pytorch_examples_amd.engine.mix import sample_trivial_augment  # noqa: E402
from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig  # noqa: E402
from dbx_distributed_pytorch_examples_amd.models import build_model  # noqa: E402
from dbx_distributed_pytorch_examples_amd.ops import kernels as K  # noqa: E402

ROOF_TBS = 6.0  # mixed read/write streaming roof used for the prediction
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out is not None:
        out.write(line + "\n")
        out.flush()


def bench_kernels(hw, batch, rounds, launches, out):
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    rs = np.random.default_rng(0)
    img = torch.randint(0, 256, (batch, hw, hw, 3), dtype=torch.uint8, generator=g).to(dev)
    x4 = torch.empty(batch, hw, hw, 4, dtype=torch.bfloat16, device=dev)
    boxes = torch.tensor([[0.0, 0.0, float(hw), float(hw)]] * batch, device=dev)
    flip = torch.randint(0, 2, (batch,), dtype=torch.uint8, generator=g).to(dev)
    perm = torch.from_numpy(rs.permutation(batch).astype("int32")).to(dev)
    none = torch.zeros(4, dtype=torch.int32, device=dev)
    one = torch.ones(1, device=dev)
    ops = torch.from_numpy(sample_trivial_augment(rs, batch, hw, hw)[1]).to(dev)
    work = torch.zeros(K.ta_work_words(batch, hw, hw), dtype=torch.int32, device=dev)
    T, hist, lut, tmean = K.ta_work_views(work, batch, hw, hw)
    K.trivial_augment_u8(img, x4, boxes, MEAN, STD, flip, ops, work)  # (fills T, the histograms, LUTs and means)
    src, t_bytes, dst = img.numel(), T.numel(), x4.numel() * 2
    calls = {
        "augment_u8 plain": (lambda: K.augment_u8(img, x4, boxes, MEAN, STD, flip), src + dst),
        "augment_u8 mixing, idle": (lambda: K.augment_u8(img, x4, boxes, MEAN, STD, flip, perm=perm, mixbox=none,
                                                         blend=one), src + dst),
        "crop_resize_u8": (lambda: K.crop_resize_u8(img, T, hist, boxes, flip), src + t_bytes),
        "ta_prepare": (lambda: K.ta_prepare(hist, ops, lut, tmean), hist.numel() * 4 + lut.numel()),
        "ta_apply_u8": (lambda: K.ta_apply_u8(T, x4, ops, lut, tmean, MEAN, STD), t_bytes + dst),
        "ta_apply_u8 mixing, idle": (lambda: K.ta_apply_u8(T, x4, ops, lut, tmean, MEAN, STD, perm=perm, mixbox=none,
                                                           blend=one), t_bytes + dst),
        "trivial_augment_u8": (lambda: K.trivial_augment_u8(img, x4, boxes, MEAN, STD, flip, ops, work),
                               src + 2 * t_bytes + dst),
    }

    def reading(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        b.synchronize()
        return 1e3 * a.elapsed_time(b) / launches

    plain = calls["augment_u8 plain"][0]
    for name, (fn, nbytes) in calls.items():
        if name == "augment_u8 plain":
            continue
        pl, vr = [], []
        for _ in range(rounds):
            pl.append(reading(plain))
            vr.append(reading(fn))
            pl.append(reading(plain))
        hist.zero_()  # (crop_resize_u8 alone accumulates)
        v = sum(vr) / len(vr)
        emit({"kernel": name, "hw": hw, "batch": batch, "launches": launches, "us": v, "us_per_round": vr,
              "plain_us": sum(pl) / len(pl), "plain_spread_within_round_us": max(abs(a - b) for a, b in zip(pl[0::2], pl[1::2])),
              "bytes": nbytes, "tb_per_s": nbytes / (v * 1e-6) / 1e12,
              "plain_tb_per_s": (src + dst) / (sum(pl) / len(pl) * 1e-6) / 1e12}, out)


def bench_model(arch, hw, batch, rounds, seconds, out):
    dev = torch.device("cuda", 0)
    classes = 1000 if hw >= 64 else 10
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (batch, hw, hw, 3), dtype=torch.uint8, generator=g).to(dev)
    lab = torch.randint(0, classes, (batch,), generator=g).to(dev)
    trs = {}
    for name, kw in (("off", {}), ("on", dict(auto_augment="ta_wide"))):
        torch.manual_seed(0)
        trs[name] = NativeTrainer(build_model(arch, num_classes=classes), batch, (hw, hw), dev,
                                  optim=OptimConfig(name="sgd", lr=0.01), label_smoothing=0.1, **kw)
        trs[name].step(img, lab)  # the resident batch; later steps reuse the static input buffers
        for _ in range(3):  # two eager warm-up steps in all, the capture, a replay
            trs[name].step()
        assert len(trs[name].graphs) == 1
    assert trs["off"].prog.ta_ops is None and trs["on"].prog.ta_ops is not None
    torch.cuda.synchronize(dev)

    def window(name, n):
        tr = trs[name]
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(n):
            tr.step()
        torch.cuda.synchronize(dev)  # (the host clock ends behind the last kernel)
        return time.perf_counter() - t0

    n = 8
    per = window("off", n) / n
    n = max(8, int(seconds / per + 7) // 8 * 8)
    readings = {"off": [], "on": []}
    for r in range(rounds):
        for slot, name in enumerate(("off", "on", "off")):
            dt = window(name, n)
            rec = {"step": True, "model": arch, "hw": hw, "batch": batch, "auto_augment": name, "round": r, "slot": slot,
                   "steps": n, "ms_per_step": 1e3 * dt / n, "img_per_s": batch * n / dt}
            readings[name].append(rec["ms_per_step"])
            emit(rec, out)
    off, on = readings["off"], readings["on"]
    m_off, m_on = sum(off) / len(off), sum(on) / len(on)
    t_bytes = batch * hw * hw * 4
    emit({"summary": True, "model": arch, "hw": hw, "batch": batch, "off_ms_per_step": m_off, "on_ms_per_step": m_on,
          "plain_vs_plain_spread_within_round_us": 1e3 * max(abs(a - b) for a, b in zip(off[0::2], off[1::2])),
          "plain_vs_plain_spread_all_us": 1e3 * (max(off) - min(off)), "on_minus_off_us": 1e3 * (m_on - m_off),
          "on_minus_off_us_per_round": [1e3 * (on[r] - 0.5 * (off[2 * r] + off[2 * r + 1])) for r in range(rounds)],
          "predicted_extra_bytes": 2 * t_bytes, "predicted_us": 2 * t_bytes / (ROOF_TBS * 1e12) * 1e6,
          "on_vs_off": m_off / m_on - 1.0}, out)
    trs.clear()
    gc.collect()
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--models", default="resnet50:224:1024,resnet18:32:256", help="arch:image size:batch, ...")
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--seconds", type=float, default=1.0, help="least duration of one step reading")
    p.add_argument("--launches", type=int, default=50)
    p.add_argument("--kernels-only", action="store_true")
    p.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = p.parse_args()
    if not torch.cuda.is_available():
        print("bench_ta: no GPU (a timing needs the device)", file=sys.stderr)
        sys.exit(2)
    out = open(a.out, "a") if a.out else None
    for spec in a.models.split(","):
        _, hw, batch = spec.split(":")
        bench_kernels(int(hw), int(batch), a.rounds, a.launches, out)
    if not a.kernels_only:
        for spec in a.models.split(","):
            arch, hw, batch = spec.split(":")
            bench_model(arch, int(hw), int(batch), a.rounds, a.seconds, out)
    if out is not None:
        out.close()


if __name__ == "__main__":
    main()
