#!/usr/bin/env python3
"""Cost of batch mixing in the native step: two NativeTrainers per model, one plain and one with MixUp +
CutMix switched per step + random erasing in "pixel" mode, on synthetic resident data, in one process,
alternated (off, on, off per round: the spread between the two "off" readings of a round is the yardstick
for on - off). One JSON line per reading (ms per step, img/s) and one summary line per model with the
measured on - off next to the prediction from bytes moved:

* a blended (MixUp) row reads its uint8 sources twice: N x Hs x Ws x C more bytes on a MixUp step, so
  ``(1 - mix_switch_prob)`` of that per step on average; a CutMix step re-reads only the box's rows (counted
  as its expected share: the mean box area of Beta(1, 1) is 1/2 of the image, its rows about 2/3);
* the output bytes are unchanged; erasing adds no bytes (erased pixels skip their gathers);
* the index_select of the second labels is one more ~5 us launch, and the host draws a few numpy
  variates and queues one small pinned copy per step (not bytes: reported as what is left over).

Then the input kernel alone per shape (``"kernel"`` records): plain against the paste, the blend, erasing and both.

  python tools/bench_mix.py [--models resnet50:224:1024,resnet18:32:256] [--rounds 3] [--out FILE]
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

ROOF_TBS = (5.9, 6.4)  # mixed read/write streaming roof, profiles/r6_roof/
LAUNCH_US = 5.0        # one more graph node (the gather of the second labels)
MIX = dict(mixup_alpha=0.2, cutmix_alpha=1.0, mix_prob=1.0, mix_switch_prob=0.5, erase_prob=0.25, erase_mode="pixel")


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out is not None:
        out.write(line + "\n")
        out.flush()


def bench_model(arch, hw, batch, rounds, seconds, out):
    dev = torch.device("cuda", 0)
    classes = 1000 if hw >= 64 else 10
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (batch, hw, hw, 3), dtype=torch.uint8, generator=g).to(dev)
    lab = torch.randint(0, classes, (batch,), generator=g).to(dev)
    trs = {}
    for name, kw in (("off", {}), ("on", MIX)):
        torch.manual_seed(0)
        trs[name] = NativeTrainer(build_model(arch, num_classes=classes), batch, (hw, hw), dev,
                                  optim=OptimConfig(name="sgd", lr=0.01), label_smoothing=0.1, **kw)
        trs[name].step(img, lab)  # the resident batch; later steps reuse the static input buffers
        for _ in range(3):  # two eager warm-up steps in all, the capture, a replay
            trs[name].step()
        assert len(trs[name].graphs) == 1
    assert trs["off"].prog.mix_blend is None and trs["on"].prog.mix_blend is not None
    torch.cuda.synchronize(dev)
    kinds = {"none": 0, "mixup": 0, "cutmix": 0}

    def window(name, n):
        tr = trs[name]
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(n):
            tr.step()
            if name == "on":
                kinds[tr.last_mix.kind] += 1
        torch.cuda.synchronize(dev)  # (the host clock ends behind the last kernel)
        return time.perf_counter() - t0

    n = 8
    per = window("off", n) / n
    n = max(8, int(seconds / per + 7) // 8 * 8)
    readings = {"off": [], "on": []}
    for r in range(rounds):
        for slot, name in enumerate(("off", "on", "off")):
            dt = window(name, n)
            rec = {"model": arch, "hw": hw, "batch": batch, "mix": name, "round": r, "slot": slot, "steps": n,
                   "ms_per_step": 1e3 * dt / n, "img_per_s": batch * n / dt}
            readings[name].append(rec["ms_per_step"])
            emit(rec, out)
    off, on = readings["off"], readings["on"]
    m_off, m_on = sum(off) / len(off), sum(on) / len(on)
    spread = max(abs(a - b) for a, b in zip(off[0::2], off[1::2]))
    src_bytes = batch * hw * hw * 3
    sw = MIX["mix_switch_prob"]
    extra = ((1.0 - sw) + sw * (2.0 / 3.0)) * src_bytes  # expected re-read per step
    pred = [extra / (tbs * 1e12) * 1e6 + LAUNCH_US for tbs in reversed(ROOF_TBS)]
    emit({"model": arch, "hw": hw, "batch": batch, "summary": True, "options": MIX, "step_kinds": kinds,
          "off_ms_per_step": m_off, "on_ms_per_step": m_on, "off_spread_within_round_us": 1e3 * spread,
          "off_spread_all_us": 1e3 * (max(off) - min(off)), "on_minus_off_us": 1e3 * (m_on - m_off),
          "on_minus_off_us_per_round": [1e3 * (on[r] - 0.5 * (off[2 * r] + off[2 * r + 1])) for r in range(rounds)],
          "source_bytes": src_bytes, "output_bytes_unchanged": batch * hw * hw * 8,
          "predicted_extra_bytes_mixup_step": src_bytes, "predicted_extra_bytes_mean": extra,
          "predicted_extra_bytes_erase": 0, "predicted_us": pred, "on_vs_off": m_off / m_on - 1.0}, out)
    trs.clear()
    import gc
    gc.collect()
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()


def bench_kernel(hw, batch, rounds, out, launches=50):
    """The input kernel alone (device events around ``launches`` launches), plain / variant / plain per round:
    the CutMix paste (plain kernel, a box of half the image), the blend (w = 0.5: every row reads two samples),
    erasing alone (w = 1; a quarter of the samples, boxes by the default rule, "pixel"), and both."""
    import numpy as np
    from dbx_distributed_pytorch_examples_amd.engine.mix import sample_erase_boxes
    from dbx_distributed_pytorch_examples_amd.ops import kernels as K
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (batch, hw, hw, 3), dtype=torch.uint8, generator=g).to(dev)
    x4 = torch.empty(batch, hw, hw, 4, dtype=torch.bfloat16, device=dev)
    boxes = torch.tensor([[0.0, 0.0, float(hw), float(hw)]] * batch, device=dev)
    flip = torch.randint(0, 2, (batch,), dtype=torch.uint8, generator=g).to(dev)
    rs = np.random.default_rng(0)
    perm = torch.from_numpy(rs.permutation(batch).astype("int32")).to(dev)
    q = int(hw * 0.5 ** 0.5)
    box = torch.tensor([0, q, 0, q], dtype=torch.int32, device=dev)
    none = torch.zeros(4, dtype=torch.int32, device=dev)
    half, one = torch.tensor([0.5], device=dev), torch.ones(1, device=dev)
    erase = torch.from_numpy(sample_erase_boxes(rs, batch, hw, hw, 0.25)).to(dev)
    rng = (1234, torch.zeros(1, dtype=torch.int32, device=dev))
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    variants = {
        "plain": {},
        "cutmix": dict(perm=perm, mixbox=box),
        "mix_idle": dict(perm=perm, mixbox=none, blend=one),  # the mixing kernel with nothing to do
        "blend": dict(perm=perm, mixbox=none, blend=half),
        "erase_pixel": dict(perm=perm, mixbox=none, blend=one, erase=erase, erase_mode="pixel", erase_rng=rng),
        "blend+erase_pixel": dict(perm=perm, mixbox=none, blend=half, erase=erase, erase_mode="pixel", erase_rng=rng),
    }

    def reading(kw):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        K.augment_u8(img, x4, boxes, mean, std, flip, **kw)
        a.record()
        for _ in range(launches):
            K.augment_u8(img, x4, boxes, mean, std, flip, **kw)
        b.record()
        b.synchronize()
        return 1e3 * a.elapsed_time(b) / launches

    src, dst = img.numel(), x4.numel() * 2
    for name, kw in variants.items():
        if name == "plain":
            continue
        pl, vr = [], []
        for _ in range(rounds):
            pl.append(reading({}))
            vr.append(reading(kw))
            pl.append(reading({}))
        emit({"kernel": "augment_u8", "variant": name, "hw": hw, "batch": batch, "launches": launches,
              "plain_us": sum(pl) / len(pl), "variant_us": sum(vr) / len(vr),
              "variant_minus_plain_us_per_round": [vr[r] - 0.5 * (pl[2 * r] + pl[2 * r + 1]) for r in range(rounds)],
              "plain_spread_within_round_us": max(abs(a - b) for a, b in zip(pl[0::2], pl[1::2])),
              "source_bytes": src, "output_bytes": dst,
              "plain_tb_per_s": (src + dst) / (sum(pl) / len(pl) * 1e-6) / 1e12}, out)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--models", default="resnet50:224:1024,resnet18:32:256", help="arch:image size:batch, ...")
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--seconds", type=float, default=1.0, help="least duration of one reading")
    p.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = p.parse_args()
    if not torch.cuda.is_available():
        print("bench_mix: no GPU (a timing needs the device)", file=sys.stderr)
        sys.exit(2)
    out = open(a.out, "a") if a.out else None
    for spec in a.models.split(","):
        arch, hw, batch = spec.split(":")
        bench_model(arch, int(hw), int(batch), a.rounds, a.seconds, out)
    for spec in a.models.split(","):
        _, hw, batch = spec.split(":")
        bench_kernel(int(hw), int(batch), a.rounds, out)
    if out is not None:
        out.close()


if __name__ == "__main__":
    main()
