#!/usr/bin/env python3
"""Cost of RandAugment (a chain of K operations) in the native step, one JSON line per record.

* ``"kernel"`` records: ``ta_stage_u8`` alone (beside ``ta_apply_u8``, which moves about the same bytes), and the
  composed ``chain_augment_u8`` at K = 2 beside the K = 1 call (``trivial_augment_u8``), per shape -- device events
  around ``--launches`` launches, reference / variant / reference per round (the two reference readings of a round
  are the spread). The table is drawn by the trainer's sampler, so the fourteen operations occur as they do in
  training. With the bytes each launch has to move and the rate that is of the time; a stage reads T once and
  writes it once, 8 bytes per pixel.
* ``"step"`` records: NativeTrainers on synthetic resident data in one process, alternated (off, ta_wide, ra, off
  per round: plain against plain is the yardstick), and a summary with the measured differences beside the
  prediction from bytes.

  python tools/bench_ra.py [--models resnet50:224:1024,resnet18:32:256] [--rounds 3] [--out FILE]
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
from dbx_distributed_pytorch_examples_amd.engine.mix import sample_rand_augment  # noqa: E402
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
    ops = torch.from_numpy(sample_rand_augment(rs, batch, hw, hw)).to(dev)  # [2, N, 8] at bin 9 of 31
    work1 = torch.zeros(K.ta_work_words(batch, hw, hw), dtype=torch.int32, device=dev)
    work = torch.zeros(K.ta_work_words(batch, hw, hw, 2), dtype=torch.int32, device=dev)
    T, hist, lut, tmean = K.ta_work_views(work, batch, hw, hw, 2)
    K.chain_augment_u8(img, x4, boxes, MEAN, STD, flip, ops, work)
    K.ta_prepare(hist[0], ops[0], lut, tmean)  # (the LUTs and means of stage 0, which the stage readings use)
    src, t_bytes, dst = img.numel(), T[0].numel(), x4.numel() * 2
    pairs = [
        ("ta_stage_u8", lambda: K.ta_stage_u8(T[0], T[1], hist[1], ops[0], lut, tmean), 2 * t_bytes,
         "ta_apply_u8", lambda: K.ta_apply_u8(T[0], x4, ops[0], lut, tmean, MEAN, STD), t_bytes + dst),
        ("chain_augment_u8 K=2", lambda: K.chain_augment_u8(img, x4, boxes, MEAN, STD, flip, ops, work),
         src + 4 * t_bytes + dst,
         "trivial_augment_u8", lambda: K.trivial_augment_u8(img, x4, boxes, MEAN, STD, flip, ops[1], work1),
         src + 2 * t_bytes + dst),
    ]

    def reading(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        b.synchronize()
        return 1e3 * a.elapsed_time(b) / launches

    for name, fn, nbytes, rname, rfn, rbytes in pairs:
        rf, vr = [], []
        for _ in range(rounds):
            rf.append(reading(rfn))
            vr.append(reading(fn))
            rf.append(reading(rfn))
        hist.zero_()  # (ta_stage_u8 alone accumulates)
        v, r = sum(vr) / len(vr), sum(rf) / len(rf)
        emit({"kernel": name, "hw": hw, "batch": batch, "launches": launches, "us": v, "us_per_round": vr,
              "reference": rname, "reference_us": r,
              "reference_spread_within_round_us": max(abs(a - b) for a, b in zip(rf[0::2], rf[1::2])),
              "bytes": nbytes, "tb_per_s": nbytes / (v * 1e-6) / 1e12, "predicted_us": nbytes / (ROOF_TBS * 1e12) * 1e6,
              "reference_bytes": rbytes, "reference_tb_per_s": rbytes / (r * 1e-6) / 1e12}, out)


def bench_model(arch, hw, batch, rounds, seconds, out):
    dev = torch.device("cuda", 0)
    classes = 1000 if hw >= 64 else 10
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (batch, hw, hw, 3), dtype=torch.uint8, generator=g).to(dev)
    lab = torch.randint(0, classes, (batch,), generator=g).to(dev)
    trs = {}
    for name, kw in (("off", {}), ("ta_wide", dict(auto_augment="ta_wide")), ("ra", dict(auto_augment="ra"))):
        torch.manual_seed(0)
        trs[name] = NativeTrainer(build_model(arch, num_classes=classes), batch, (hw, hw), dev,
                                  optim=OptimConfig(name="sgd", lr=0.01), label_smoothing=0.1, **kw)
        trs[name].step(img, lab)  # the resident batch; later steps reuse the static input buffers
        for _ in range(3):  # two eager warm-up steps in all, the capture, a replay
            trs[name].step()
        assert len(trs[name].graphs) == 1
    assert trs["off"].prog.ta_ops is None and trs["ta_wide"].prog.ta_stages == 1 and trs["ra"].prog.ta_stages == 2
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
    readings = {"off": [], "ta_wide": [], "ra": []}
    for r in range(rounds):
        for slot, name in enumerate(("off", "ta_wide", "ra", "off")):
            dt = window(name, n)
            rec = {"step": True, "model": arch, "hw": hw, "batch": batch, "auto_augment": name, "round": r, "slot": slot,
                   "steps": n, "ms_per_step": 1e3 * dt / n, "img_per_s": batch * n / dt}
            readings[name].append(rec["ms_per_step"])
            emit(rec, out)
    off, ta, ra = readings["off"], readings["ta_wide"], readings["ra"]
    m_off, m_ta, m_ra = (sum(v) / len(v) for v in (off, ta, ra))
    t_bytes = batch * hw * hw * 4
    emit({"summary": True, "model": arch, "hw": hw, "batch": batch, "off_ms_per_step": m_off, "ta_wide_ms_per_step": m_ta,
          "ra_ms_per_step": m_ra,
          "plain_vs_plain_spread_within_round_us": 1e3 * max(abs(a - b) for a, b in zip(off[0::2], off[1::2])),
          "plain_vs_plain_spread_all_us": 1e3 * (max(off) - min(off)), "ra_minus_off_us": 1e3 * (m_ra - m_off),
          "ra_minus_ta_wide_us": 1e3 * (m_ra - m_ta),
          "ra_minus_ta_wide_us_per_round": [1e3 * (ra[r] - ta[r]) for r in range(rounds)],
          "predicted_extra_bytes_over_ta_wide": 2 * t_bytes, "predicted_us": 2 * t_bytes / (ROOF_TBS * 1e12) * 1e6,
          "ra_vs_off": m_off / m_ra - 1.0, "ra_vs_ta_wide": m_ta / m_ra - 1.0}, out)
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
        print("bench_ra: no GPU (a timing needs the device)", file=sys.stderr)
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
