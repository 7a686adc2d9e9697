#!/usr/bin/env python3
"""Cost of the weight EMA in the native step: two NativeTrainers per model, ema_decay 0 and 0.9999, on
synthetic resident data, in one process, alternated (off, on, off per round: the spread between the
two "off" readings of a round is the yardstick for on - off). One JSON line per reading (ms per step,
img/s) and one summary line per model with the measured on - off next to the prediction from bytes
moved: 8 B x n_params more traffic in the optimizer kernel at the probed 5.9-6.4 TB/s mixed
read/write roof (profiles/r6_roof/) plus one ~5 us launch for the BN running statistics.
  python tools/bench_ema.py [--models resnet50:224:1024,resnet18:32:256] [--rounds 3] [--out FILE]
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
LAUNCH_US = 5.0        # one more graph node (the BN-statistics launch)


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out is not None:
        out.write(line + "\n")
        out.flush()


def bench_model(arch, hw, batch, rounds, seconds, optim, out):
    dev = torch.device("cuda", 0)
    classes = 1000 if hw >= 64 else 10
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (batch, hw, hw, 3), dtype=torch.uint8, generator=g).to(dev)
    lab = torch.randint(0, classes, (batch,), generator=g).to(dev)
    trs = {}
    for name, decay in (("off", 0.0), ("on", 0.9999)):
        torch.manual_seed(0)
        trs[name] = NativeTrainer(build_model(arch, num_classes=classes), batch, (hw, hw), dev,
                                  optim=OptimConfig(name=optim, lr=0.01 if optim == "sgd" else 1e-3),
                                  ema_decay=decay)  # (constant decay: no per-step refresh of 1 - d_t)
        trs[name].step(img, lab)  # the resident batch; later steps reuse the static input buffers
        for _ in range(3):  # two eager warm-up steps in all, the capture, a replay
            trs[name].step()
        assert len(trs[name].graphs) == 1
    assert trs["off"].ema is None and trs["on"].ema is not None
    n_params = trs["on"].prog.n_params
    n_bn = trs["on"]._ema_bn_n
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
            rec = {"model": arch, "hw": hw, "batch": batch, "optim": optim, "ema": name, "round": r, "slot": slot,
                   "steps": n, "ms_per_step": 1e3 * dt / n, "img_per_s": batch * n / dt}
            readings[name].append(rec["ms_per_step"])
            emit(rec, out)
    off, on = readings["off"], readings["on"]
    m_off, m_on = sum(off) / len(off), sum(on) / len(on)
    spread = max(abs(a - b) for a, b in zip(off[0::2], off[1::2]))
    pred = [8.0 * n_params / (tbs * 1e12) * 1e6 + LAUNCH_US for tbs in reversed(ROOF_TBS)]
    emit({"model": arch, "hw": hw, "batch": batch, "optim": optim, "summary": True, "n_params": n_params,
          "bn_buffers": n_bn, "off_ms_per_step": m_off, "on_ms_per_step": m_on,
          "off_spread_within_round_us": 1e3 * spread, "off_spread_all_us": 1e3 * (max(off) - min(off)),
          "on_minus_off_us": 1e3 * (m_on - m_off),
          "on_minus_off_us_per_round": [1e3 * (on[r] - 0.5 * (off[2 * r] + off[2 * r + 1])) for r in range(rounds)],
          "predicted_us": pred, "on_vs_off": m_off / m_on - 1.0}, out)
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
    p.add_argument("--optim", default="sgd", choices=("sgd", "adamw", "lars"))
    p.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = p.parse_args()
    if not torch.cuda.is_available():
        print("bench_ema: no GPU (a timing needs the device)", file=sys.stderr)
        sys.exit(2)
    out = open(a.out, "a") if a.out else None
    for spec in a.models.split(","):
        arch, hw, batch = spec.split(":")
        bench_model(arch, int(hw), int(batch), a.rounds, a.seconds, a.optim, out)
    if out is not None:
        out.close()


if __name__ == "__main__":
    main()
