#!/usr/bin/env python3
"""Cost of the resampling filters, one JSON line per record.

* ``"kernel"`` records: ``resample_u8_kernel`` against the bilinear kernel of the same entry point on the same boxes
  (RandomResizedCrop boxes and flips, random bytes), alternated bilinear / filter / bilinear per round in one process
  (the two bilinear readings of a round are the spread), for each filter and both modes (``image``: ``augment_u8``;
  ``T``: ``crop_resize_u8``). Cases: dense ``SxS -> hw`` and ``mix``: a seeded ragged mix of shorter side S. With the
  prediction stated before measuring -- the bytes are the bilinear kernel's, the added cost is arithmetic,
  ``(1 + 2 S fs / (kRows scale)) Tx + Ty`` multiply-adds per output value (Tx = Ty = 2 S fs taps, averaged over the
  boxes) -- next to the measured added time per output value.
* ``"step"`` records: a NativeTrainer with ``resample="aa_bicubic"`` against one with None on the same resident batch,
  alternated (None, filter, None per round), and a summary.

  python tools/bench_resample.py [--cases 256:224:1024:dense,480:224:1024:mix,40:32:256:dense]
                                 [--models resnet50:224:1024,resnet18:32:256] [--rounds 3] [--out FILE]
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
from bench_ragged import ASPECTS, MEAN, RRC, STD, emit, reading  # noqa: E402
from dbx_distributed_pytorch_examples_amd.data.loader import pack_layout, sample_boxes  # noqa: E402
from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig  # noqa: E402
from dbx_distributed_pytorch_examples_amd.models import build_model  # noqa: E402
from dbx_distributed_pytorch_examples_amd.ops import kernels as K  # noqa: E402

FILTERS = ("aa_bilinear", "bicubic", "aa_bicubic")
K_ROWS = 16  # csrc/input_resample.hip kRsRows


def predicted_mads(boxes, hw, name):
    """The stated prediction, averaged over the boxes: multiply-adds per output value."""
    S, aa = (1.0 if name == "aa_bilinear" else 2.0), name != "bicubic"
    sy, sx = boxes[:, 2] / hw, boxes[:, 3] / hw
    fy, fx = (np.maximum(sy, 1.0), np.maximum(sx, 1.0)) if aa else (np.ones_like(sy), np.ones_like(sx))
    return float(np.mean((1.0 + 2.0 * S * fy / (K_ROWS * sy)) * 2.0 * S * fx + 2.0 * S * fy))


def bench_kernels(side, hw, batch, mixed, rounds, launches, out):
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    rs = np.random.default_rng(0)
    if mixed:
        asp = [ASPECTS[i] for i in rs.integers(0, len(ASPECTS), batch)]
        hs = np.array([side if aw >= ah else side * ah // aw for aw, ah in asp])
        ws = np.array([side * aw // ah if aw >= ah else side for aw, ah in asp])
        table, used = pack_layout(hs, ws, 3)
        img = torch.randint(0, 256, (max(used, 16),), dtype=torch.uint8, generator=g).to(dev)
        src = dict(src=torch.from_numpy(table).to(dev), src_channels=3)
    else:
        hs, ws, src = side, side, {}
        img = torch.randint(0, 256, (batch, side, side, 3), dtype=torch.uint8, generator=g).to(dev)
    box_np, flips = sample_boxes(batch, hs, ws, hw, hw, RRC, random.Random(0))
    boxes, flip = torch.from_numpy(box_np).to(dev), torch.from_numpy(flips).to(dev)
    x4 = torch.empty(batch, hw, hw, 4, dtype=torch.bfloat16, device=dev)
    T = torch.empty(batch, hw, hw, 4, dtype=torch.uint8, device=dev)
    hist = torch.zeros(batch, 4, 256, dtype=torch.int32, device=dev)
    values = 3 * batch * hw * hw
    for name in FILTERS:
        for mode, call in (("image", lambda rsm: K.augment_u8(img, x4, boxes, MEAN, STD, flip, resample=rsm, **src)),
                           ("T", lambda rsm: K.crop_resize_u8(img, T, hist, boxes, flip, resample=rsm, **src))):
            base, new = [], []
            for _ in range(rounds):
                base.append(reading(lambda: call(None), launches))
                new.append(reading(lambda: call(name), launches))
                base.append(reading(lambda: call(None), launches))
            hist.zero_()
            b, n = sum(base) / len(base), sum(new) / len(new)
            mads = predicted_mads(box_np, hw, name)
            emit({"kernel": "resample_u8", "filter": name, "mode": mode, "batch": batch, "launches": launches,
                  "case": f"{'ragged mix' if mixed else 'dense'} {side} -> {hw}", "bilinear_us": b, "filter_us": n,
                  "filter_over_bilinear": n / b, "filter_us_per_round": new,
                  "bilinear_spread_within_round_us": max(abs(x - y) for x, y in zip(base[0::2], base[1::2])),
                  "predicted_mads_per_output_value": mads, "added_ns_per_output_value": 1e3 * (n - b) / values,
                  "added_time_as_gmads_per_s": mads * values / (1e3 * (n - b)) if n > b else None}, out)


def bench_model(arch, hw, batch, rounds, seconds, out):
    dev = torch.device("cuda", 0)
    classes, side = (1000, 256) if hw >= 64 else (10, 40)
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (batch, side, side, 3), dtype=torch.uint8, generator=g).to(dev)
    lab = torch.randint(0, classes, (batch,), generator=g).to(dev)
    boxes, flips = sample_boxes(batch, side, side, hw, hw, RRC, random.Random(0))
    boxes, flips = torch.from_numpy(boxes).to(dev), torch.from_numpy(flips).to(dev)
    trs = {}
    for name in (None, "aa_bicubic"):
        torch.manual_seed(0)
        trs[name] = tr = NativeTrainer(build_model(arch, num_classes=classes), batch, (hw, hw), dev, src_hw=(side, side),
                                       optim=OptimConfig(name="sgd", lr=0.01), label_smoothing=0.1, resample=name)
        tr.step(img, lab, boxes, flips)
        for _ in range(3):  # two eager warm-up steps in all, the capture, a replay
            tr.step()
        assert len(tr.graphs) == 1

    def window(name, n):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(n):
            trs[name].step()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0

    n = max(8, int(seconds / (window(None, 8) / 8) + 7) // 8 * 8)
    ms = {None: [], "aa_bicubic": []}
    for r in range(rounds):
        for slot, name in enumerate((None, "aa_bicubic", None)):
            dt = window(name, n)
            ms[name].append(1e3 * dt / n)
            emit({"step": True, "model": arch, "hw": hw, "batch": batch, "resample": name, "round": r, "slot": slot,
                  "steps": n, "ms_per_step": 1e3 * dt / n, "img_per_s": batch * n / dt}, out)
    b, f = ms[None], ms["aa_bicubic"]
    m_b, m_f = sum(b) / len(b), sum(f) / len(f)
    emit({"summary": True, "model": arch, "hw": hw, "batch": batch, "src": side, "bilinear_ms_per_step": m_b,
          "aa_bicubic_ms_per_step": m_f, "aa_bicubic_minus_bilinear_us": 1e3 * (m_f - m_b),
          "bilinear_spread_within_round_us": 1e3 * max(abs(x - y) for x, y in zip(b[0::2], b[1::2])),
          "bilinear_spread_all_us": 1e3 * (max(b) - min(b)), "aa_bicubic_vs_bilinear": m_b / m_f - 1.0}, out)
    trs.clear()
    gc.collect()
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--cases", default="256:224:1024:dense,480:224:1024:mix,40:32:256:dense",
                   help="source side:output size:batch:dense|mix, ...")
    p.add_argument("--models", default="resnet50:224:1024,resnet18:32:256", help="arch:image size:batch, ...")
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--seconds", type=float, default=1.0, help="least duration of one step reading")
    p.add_argument("--launches", type=int, default=20)
    p.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = p.parse_args()
    if not torch.cuda.is_available():
        print("bench_resample: no GPU (a timing needs the device)", file=sys.stderr)
        sys.exit(2)
    out = open(a.out, "a") if a.out else None
    for spec in filter(None, a.cases.split(",")):
        side, hw, batch, kind = spec.split(":")
        bench_kernels(int(side), int(hw), int(batch), kind == "mix", a.rounds, a.launches, out)
    for spec in filter(None, a.models.split(",")):
        arch, hw, batch = spec.split(":")
        bench_model(arch, int(hw), int(batch), a.rounds, a.seconds, out)
    if out is not None:
        out.close()


if __name__ == "__main__":
    main()
