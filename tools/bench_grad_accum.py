#!/usr/bin/env python3
"""Cost of gradient accumulation in the native step: NativeTrainers with grad_accum k in {1, 2, 8} on
synthetic resident data, in one process, timed in whole windows and alternated (k = 1, the plain
step, is read twice per round: the spread between its two readings is the yardstick for the others).
One JSON line per reading (img/s, ms per micro-step) and one summary line per model.
  python tools/bench_grad_accum.py [--models resnet50:224:1024,resnet18:32:256] [--rounds 3] [--out FILE]
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

KS = (1, 2, 8)


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
    for k in KS:
        torch.manual_seed(0)
        trs[k] = NativeTrainer(build_model(arch, num_classes=classes), batch, (hw, hw), dev,
                               optim=OptimConfig(name="sgd", lr=0.01), grad_accum=k)
        trs[k].step(img, lab)  # the resident batch; later steps reuse the static input buffers
        # every graph kind, in four windows: two eager warm-up steps, the capture, a replay
        for _ in range(4 * k - 1):
            trs[k].step()
        assert trs[k].micro == 0 and len(trs[k].graphs) == 1 and len(trs[k].micro_graphs) == (k > 1)
    torch.cuda.synchronize(dev)

    def window(k, n):
        tr = trs[k]
        assert tr.micro == 0 and n % k == 0
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(n):
            tr.step()
        torch.cuda.synchronize(dev)  # (the host clock ends behind the last kernel)
        return time.perf_counter() - t0

    # micro-steps per reading: a multiple of every k, long enough to time (>= ``seconds``)
    n = 8
    per = window(1, n) / n
    n = max(8, int(seconds / per + 7) // 8 * 8)
    readings = {k: [] for k in KS}
    for r in range(rounds):
        for slot, k in enumerate((1, 2, 8, 1)):
            dt = window(k, n)
            rec = {"model": arch, "hw": hw, "batch": batch, "optim": "sgd", "k": k, "round": r, "slot": slot,
                   "micro_steps": n, "ms_per_micro_step": 1e3 * dt / n, "img_per_s": batch * n / dt}
            readings[k].append((r, rec["img_per_s"]))
            emit(rec, out)
    # the spread of the interleaved k = 1 readings (per round: its two readings), and each k against k = 1
    k1 = [v for _, v in readings[1]]
    mean1 = sum(k1) / len(k1)
    spread = max(abs(a - b) for (ra, a), (rb, b) in zip(readings[1][0::2], readings[1][1::2])) / mean1
    summ = {"model": arch, "hw": hw, "batch": batch, "summary": True, "k1_img_per_s": mean1,
            "k1_spread_within_round": spread, "k1_spread_all": (max(k1) - min(k1)) / mean1}
    for k in KS[1:]:
        mk = sum(v for _, v in readings[k]) / len(readings[k])
        summ[f"k{k}_img_per_s"] = mk
        summ[f"k{k}_vs_k1"] = mk / mean1 - 1.0
    emit(summ, out)
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
    p.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = p.parse_args()
    if not torch.cuda.is_available():
        print("bench_grad_accum: no GPU (a timing needs the device)", file=sys.stderr)
        sys.exit(2)
    out = open(a.out, "a") if a.out else None
    for spec in a.models.split(","):
        arch, hw, batch = spec.split(":")
        bench_model(arch, int(hw), int(batch), a.rounds, a.seconds, out)
    if out is not None:
        out.close()


if __name__ == "__main__":
    main()
