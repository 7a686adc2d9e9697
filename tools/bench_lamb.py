#!/usr/bin/env python3
"""Cost of LAMB in the native step: two NativeTrainers per model, ``adamw`` and ``lamb``, on synthetic
resident data, in one process, alternated (adamw, lamb, adamw per round: the spread between the two
adamw readings of a round is the yardstick for lamb - adamw). One JSON line per reading (ms per step,
img/s) and one summary line per model with the measured lamb - adamw next to the prediction from bytes
moved: the two LAMB kernels move 40 B per parameter (moments: read w, g, m, v, write m, v, u = 28 B;
apply: read w, u, write w = 12 B) against Adam's 28 B (+ 8 B each with the weight EMA, ``--ema``), over
``n_params`` at the probed 5.9-6.4 TB/s mixed read/write roof (profiles/r6_roof/), plus one ~5 us
launch (two kernels instead of one). adamw updates inside the backward (``overlap_optimizer``) while
LAMB's per-tensor norms keep its update behind the backward, so part of a difference is the schedule,
not the bytes: ``--serial-adamw`` gives adamw a clip that never clips (grad_clip 1e30), which moves its
update to the optimizer phase too at the price of one norm pass (4 B per parameter, subtracted from the
prediction).
  python tools/bench_lamb.py [--models resnet50:224:1024,resnet18:32:256] [--rounds 3] [--ema] [--out FILE]
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
LAUNCH_US = 5.0        # one more graph node (two kernels against Adam's one)
LAMB_BYTES, ADAM_BYTES, NORM_BYTES = 40.0, 28.0, 4.0


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out is not None:
        out.write(line + "\n")
        out.flush()


def bench_model(arch, hw, batch, rounds, seconds, ema, serial_adamw, out):
    dev = torch.device("cuda", 0)
    classes = 1000 if hw >= 64 else 10
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (batch, hw, hw, 3), dtype=torch.uint8, generator=g).to(dev)
    lab = torch.randint(0, classes, (batch,), generator=g).to(dev)
    trs = {}
    for name in ("adamw", "lamb"):
        torch.manual_seed(0)
        clip = 1e30 if (serial_adamw and name == "adamw") else 0.0
        trs[name] = NativeTrainer(build_model(arch, num_classes=classes), batch, (hw, hw), dev,
                                  optim=OptimConfig(name=name, lr=1e-3, weight_decay=0.01, grad_clip=clip),
                                  ema_decay=0.9999 if ema else 0.0)
        trs[name].step(img, lab)  # the resident batch; later steps reuse the static input buffers
        for _ in range(3):  # two eager warm-up steps in all, the capture, a replay
            trs[name].step()
        assert len(trs[name].graphs) == 1
    assert trs["lamb"].lamb is not None and trs["adamw"].lamb is None
    n_params = trs["lamb"].prog.n_params
    adamw_in_backward = trs["adamw"].opt_ranges is not None
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
    per = window("adamw", n) / n
    n = max(8, int(seconds / per + 7) // 8 * 8)
    readings = {"adamw": [], "lamb": []}
    for r in range(rounds):
        for slot, name in enumerate(("adamw", "lamb", "adamw")):
            dt = window(name, n)
            rec = {"model": arch, "hw": hw, "batch": batch, "optim": name, "ema": bool(ema), "round": r, "slot": slot,
                   "steps": n, "ms_per_step": 1e3 * dt / n, "img_per_s": batch * n / dt}
            readings[name].append(rec["ms_per_step"])
            emit(rec, out)
    base, lamb = readings["adamw"], readings["lamb"]
    m_base, m_lamb = sum(base) / len(base), sum(lamb) / len(lamb)
    spread = max(abs(a - b) for a, b in zip(base[0::2], base[1::2]))
    extra = LAMB_BYTES - ADAM_BYTES - (NORM_BYTES if serial_adamw else 0.0)  # (the EMA's 8 B are on both sides)
    pred = [extra * n_params / (tbs * 1e12) * 1e6 + LAUNCH_US for tbs in reversed(ROOF_TBS)]
    emit({"model": arch, "hw": hw, "batch": batch, "ema": bool(ema), "summary": True, "n_params": n_params,
          "adamw_updates_inside_backward": adamw_in_backward, "serial_adamw": bool(serial_adamw),
          "bytes_per_param": {"lamb": LAMB_BYTES + (8.0 if ema else 0.0), "adamw": ADAM_BYTES + (8.0 if ema else 0.0)},
          "adamw_ms_per_step": m_base, "lamb_ms_per_step": m_lamb,
          "adamw_spread_within_round_us": 1e3 * spread, "adamw_spread_all_us": 1e3 * (max(base) - min(base)),
          "lamb_minus_adamw_us": 1e3 * (m_lamb - m_base),
          "lamb_minus_adamw_us_per_round": [1e3 * (lamb[r] - 0.5 * (base[2 * r] + base[2 * r + 1]))
                                            for r in range(rounds)],
          "predicted_us": pred, "lamb_vs_adamw": m_base / m_lamb - 1.0}, out)
    trs.clear()
    import gc
    gc.collect()
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--models", default="resnet50:224:1024,resnet18:32:256", help="arch:image size:batch, ...")
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--seconds", type=float, default=1.0, help="least duration of one reading")
    p.add_argument("--ema", action="store_true", help="both trainers with ema_decay=0.9999 (the fused-EMA variants)")
    p.add_argument("--serial-adamw", action="store_true",
                   help="adamw with grad_clip=1e30: its update behind the backward, like LAMB's")
    p.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = p.parse_args()
    if not torch.cuda.is_available():
        print("bench_lamb: no GPU (a timing needs the device)", file=sys.stderr)
        sys.exit(2)
    out = open(a.out, "a") if a.out else None
    for spec in a.models.split(","):
        arch, hw, batch = spec.split(":")
        bench_model(arch, int(hw), int(batch), a.rounds, a.seconds, a.ema, a.serial_adamw, out)
    if out is not None:
        out.close()


if __name__ == "__main__":
    main()
