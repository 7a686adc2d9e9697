#!/usr/bin/env python3
"""Cost of ragged input batches, one JSON line per record.

* ``"kernel"`` records: each of the three input kernels that read the source (``augment_u8``, its mixing form
  with a MixUp blend, ``crop_resize_u8``) on a dense batch and on a ragged source of the same sizes (random bytes),
  alternated dense / ragged / dense per round (the two dense readings of a round are the spread), with
  RandomResizedCrop boxes and flips. Cases: uniform ``SxS -> hw``, and ``mix``: a seeded mix of shorter side S
  with aspects 3:4, 1:1, 4:3, 3:2, 16:9, whose dense counterpart is the same batch squashed to ``SxS`` at write
  time (the only way round without ragged batches). With the host-to-device bytes of either form.
* ``"step"`` records: a ragged NativeTrainer against a dense one on the same resident uniform batch in one
  process, alternated (dense, ragged, dense per round), and a summary.

  python tools/bench_ragged.py [--cases 256:224:1024,40:32:256] [--models resnet50:224:1024,resnet18:32:256]
                               [--rounds 3] [--out FILE]
"""
import argparse
import gc
import json
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dbx_distributed_pytorch_examples_amd.data.loader import AugmentSpec, pack_layout, sample_boxes  # noqa: E402
from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig  # noqa: E402
from dbx_distributed_pytorch_examples_amd.models import build_model  # noqa: E402
from dbx_distributed_pytorch_examples_amd.ops import kernels as K  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
ASPECTS = [(3, 4), (1, 1), (4, 3), (3, 2), (16, 9)]  # width : height
RRC = AugmentSpec(mode="random_resized_crop", hflip=True)


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out is not None:
        out.write(line + "\n")
        out.flush()


def reading(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / launches


def random_arena(table, used, dev, g):
    """A random-byte arena for ``table`` (the padding bytes are never read as pixels)."""
    return torch.randint(0, 256, (max(used, 16),), dtype=torch.uint8, generator=g).to(dev)


def bench_kernels(side, hw, batch, mixed, rounds, launches, out):
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    rs = np.random.default_rng(0)
    if mixed:
        asp = [ASPECTS[i] for i in rs.integers(0, len(ASPECTS), batch)]
        hs = np.array([side if aw >= ah else side * ah // aw for aw, ah in asp])
        ws = np.array([side * aw // ah if aw >= ah else side for aw, ah in asp])
    else:
        hs, ws = np.full(batch, side), np.full(batch, side)
    table, used = pack_layout(hs, ws, 3)
    arena = random_arena(table, used, dev, g)
    tab = torch.from_numpy(table).to(dev)
    dense = torch.randint(0, 256, (batch, side, side, 3), dtype=torch.uint8, generator=g).to(dev)
    rbox, flips = sample_boxes(batch, hs, ws, hw, hw, RRC, random.Random(0))
    dbox, _ = sample_boxes(batch, side, side, hw, hw, RRC, random.Random(0))
    rbox, dbox, flip = (torch.from_numpy(a).to(dev) for a in (rbox, dbox, flips))
    x4 = torch.empty(batch, hw, hw, 4, dtype=torch.bfloat16, device=dev)
    T = torch.empty(batch, hw, hw, 4, dtype=torch.uint8, device=dev)
    hist = torch.zeros(batch, 4, 256, dtype=torch.int32, device=dev)
    perm = torch.from_numpy(rs.permutation(batch).astype("int32")).to(dev)
    w = torch.tensor([0.3], device=dev)
    src = dict(src=tab, src_channels=3)
    calls = {
        "augment_u8": (lambda: K.augment_u8(dense, x4, dbox, MEAN, STD, flip),
                       lambda: K.augment_u8(arena, x4, rbox, MEAN, STD, flip, **src)),
        "augment_mix_u8 blend": (lambda: K.augment_u8(dense, x4, dbox, MEAN, STD, flip, perm=perm, blend=w),
                                 lambda: K.augment_u8(arena, x4, rbox, MEAN, STD, flip, perm=perm, blend=w, **src)),
        "crop_resize_u8": (lambda: K.crop_resize_u8(dense, T, hist, dbox, flip),
                           lambda: K.crop_resize_u8(arena, T, hist, rbox, flip, **src)),
    }
    for name, (fd, fr) in calls.items():
        dn, rg = [], []
        for _ in range(rounds):
            dn.append(reading(fd, launches))
            rg.append(reading(fr, launches))
            dn.append(reading(fd, launches))
        hist.zero_()
        d, r = sum(dn) / len(dn), sum(rg) / len(rg)
        emit({"kernel": name, "case": f"{'mix' if mixed else 'uniform'} {side} -> {hw}", "batch": batch,
              "launches": launches, "dense_us": d, "ragged_us": r, "ragged_over_dense": r / d, "ragged_us_per_round": rg,
              "dense_spread_within_round_us": max(abs(a - b) for a, b in zip(dn[0::2], dn[1::2])),
              "h2d_bytes_dense": dense.numel(), "h2d_bytes_packed": used + tab.numel() * 4,
              "packed_over_dense_bytes": (used + tab.numel() * 4) / dense.numel()}, out)


def bench_model(arch, hw, batch, rounds, seconds, out):
    dev = torch.device("cuda", 0)
    classes = 1000 if hw >= 64 else 10
    side = 256 if hw >= 64 else 40
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (batch, side, side, 3), dtype=torch.uint8, generator=g).to(dev)
    lab = torch.randint(0, classes, (batch,), generator=g).to(dev)
    table, used = pack_layout([side] * batch, [side] * batch, 3)
    arena = torch.zeros(used, dtype=torch.uint8, device=dev)  # the same pixels, rows padded to the table's stride
    arena.view(batch, side, int(table[0, 3]))[:, :, :side * 3] = img.view(batch, side, side * 3)
    boxes, flips = sample_boxes(batch, side, side, hw, hw, RRC, random.Random(0))
    boxes, flips = torch.from_numpy(boxes).to(dev), torch.from_numpy(flips).to(dev)
    trs = {}
    for name, kw in (("dense", dict(src_hw=(side, side))), ("ragged", dict(src_ragged=(side, side)))):
        torch.manual_seed(0)
        trs[name] = tr = NativeTrainer(build_model(arch, num_classes=classes), batch, (hw, hw), dev,
                                       optim=OptimConfig(name="sgd", lr=0.01), label_smoothing=0.1, **kw)
        if name == "dense":
            tr.step(img, lab, boxes, flips)
        else:
            tr.step(arena, lab, boxes, flips, src_table=torch.from_numpy(table).to(dev))
        for _ in range(3):  # two eager warm-up steps in all, the capture, a replay
            tr.step()
        assert len(tr.graphs) == 1
    same = torch.equal(trs["dense"].prog.x4, trs["ragged"].prog.x4) and torch.equal(trs["dense"].prog.master,
                                                                                    trs["ragged"].prog.master)
    torch.cuda.synchronize(dev)

    def window(name, n):
        tr = trs[name]
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(n):
            tr.step()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0

    n = 8
    per = window("dense", n) / n
    n = max(8, int(seconds / per + 7) // 8 * 8)
    readings = {"dense": [], "ragged": []}
    for r in range(rounds):
        for slot, name in enumerate(("dense", "ragged", "dense")):
            dt = window(name, n)
            rec = {"step": True, "model": arch, "hw": hw, "batch": batch, "source": name, "round": r, "slot": slot,
                   "steps": n, "ms_per_step": 1e3 * dt / n, "img_per_s": batch * n / dt}
            readings[name].append(rec["ms_per_step"])
            emit(rec, out)
    dn, rg = readings["dense"], readings["ragged"]
    m_d, m_r = sum(dn) / len(dn), sum(rg) / len(rg)
    emit({"summary": True, "model": arch, "hw": hw, "batch": batch, "src": side, "dense_ms_per_step": m_d,
          "ragged_ms_per_step": m_r, "ragged_minus_dense_us": 1e3 * (m_r - m_d),
          "dense_vs_dense_spread_within_round_us": 1e3 * max(abs(a - b) for a, b in zip(dn[0::2], dn[1::2])),
          "dense_vs_dense_spread_all_us": 1e3 * (max(dn) - min(dn)), "ragged_vs_dense": m_d / m_r - 1.0,
          "bit_identical_after_4_steps": bool(same)}, out)
    trs.clear()
    gc.collect()
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--cases", default="256:224:1024,40:32:256", help="source side:output size:batch, ...")
    p.add_argument("--models", default="resnet50:224:1024,resnet18:32:256", help="arch:image size:batch, ...")
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--seconds", type=float, default=1.0, help="least duration of one step reading")
    p.add_argument("--launches", type=int, default=50)
    p.add_argument("--kernels-only", action="store_true")
    p.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = p.parse_args()
    if not torch.cuda.is_available():
        print("bench_ragged: no GPU (a timing needs the device)", file=sys.stderr)
        sys.exit(2)
    out = open(a.out, "a") if a.out else None
    for spec in a.cases.split(","):
        side, hw, batch = (int(v) for v in spec.split(":"))
        bench_kernels(side, hw, batch, False, a.rounds, a.launches, out)
        if side >= 128:
            bench_kernels(side, hw, batch, True, a.rounds, a.launches, out)
    if not a.kernels_only:
        for spec in a.models.split(","):
            arch, hw, batch = spec.split(":")
            bench_model(arch, int(hw), int(batch), a.rounds, a.seconds, out)
    if out is not None:
        out.close()


if __name__ == "__main__":
    main()
