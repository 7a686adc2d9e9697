#!/usr/bin/env python3
"""Cost of binary cross-entropy as the training loss, next to softmax cross-entropy.

* ``kernels``: ``K.bce_logits`` against ``K.softmax_ce`` alone, each with dlogits and the two counters, in a
  captured graph of ``--launches`` back-to-back launches (so the reading is device time per launch, not the host's
  enqueue), alternated ce, bce, ce per round. The prediction printed beside each reading: both kernels read the
  logits and write dlogits once, ``2 B C sizeof(T)`` bytes -- 4.1 MB at (1024, 1000) bf16, 0.7 us at the probed
  5.9-6.4 TB/s roof (profiles/r6_roof/) -- so both are launch latency (a few us), not bandwidth.
* ``steps``: two NativeTrainers per model, ``loss="ce"`` and ``loss="bce"``, on synthetic resident data, in one
  process, alternated ce, bce, ce per round (the spread between the two ce readings of a round is the yardstick
  for bce - ce). The prediction: one launch replaces one launch inside the captured step, 0 +- the spread.
  python tools/bench_bce.py [--models resnet18:32:256,resnet50:224:1024] [--rounds 3] [--out FILE]
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

ROOF_TBS = (5.9, 6.4)  # mixed read/write streaming roof, profiles/r6_roof/
KERNEL_SHAPES = ((1024, 1000), (256, 10))


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out is not None:
        out.write(line + "\n")
        out.flush()


def bench_kernels(B, C, rounds, launches, out):
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(B, C, generator=g) * 2.0).to(dev).bfloat16()
    lab = torch.randint(0, C, (B,), generator=g).to(dev)
    dl = torch.empty_like(x)
    st = torch.zeros(2, device=dev, dtype=torch.float64)
    fns = {"ce": lambda: K.softmax_ce(x, lab, dl, None, st, smoothing=0.1),
           "bce": lambda: K.bce_logits(x, lab, dl, None, st, smoothing=0.1)}
    graphs = {}
    for name, fn in fns.items():
        fn()
        torch.cuda.synchronize(dev)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(launches):
                fn()
        graphs[name] = gr
        gr.replay()
    torch.cuda.synchronize(dev)

    def window(name, reps=20):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(reps):
            graphs[name].replay()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / (reps * launches)

    nbytes = 2 * B * C * x.element_size()
    pred = [nbytes / (tbs * 1e12) * 1e6 for tbs in reversed(ROOF_TBS)]
    readings = {"ce": [], "bce": []}
    for r in range(rounds):
        for slot, name in enumerate(("ce", "bce", "ce")):
            us = 1e6 * window(name)
            readings[name].append(us)
            emit({"kernel": "softmax_ce" if name == "ce" else "bce_logits", "B": B, "C": C, "dtype": "bf16", "round": r,
                  "slot": slot, "launches_per_graph": launches, "us_per_launch": us, "bytes": nbytes,
                  "predicted_us_at_the_roof": pred}, out)
    ce, bce = readings["ce"], readings["bce"]
    emit({"summary": "kernels", "B": B, "C": C, "dtype": "bf16", "bytes": nbytes, "predicted_us_at_the_roof": pred,
          "prediction": "both are launch latency: a few us each, far above the bytes' time",
          "softmax_ce_us": sum(ce) / len(ce), "bce_logits_us": sum(bce) / len(bce),
          "softmax_ce_spread_us": max(ce) - min(ce), "bce_minus_ce_us": sum(bce) / len(bce) - sum(ce) / len(ce)}, out)


def bench_model(arch, hw, batch, rounds, seconds, out):
    dev = torch.device("cuda", 0)
    classes = 1000 if hw >= 64 else 10
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (batch, hw, hw, 3), dtype=torch.uint8, generator=g).to(dev)
    lab = torch.randint(0, classes, (batch,), generator=g).to(dev)
    trs = {}
    for name in ("ce", "bce"):
        torch.manual_seed(0)
        trs[name] = NativeTrainer(build_model(arch, num_classes=classes), batch, (hw, hw), dev,
                                  optim=OptimConfig(lr=1e-3), label_smoothing=0.1, loss=name)
        trs[name].step(img, lab)  # the resident batch; later steps reuse the static input buffers
        for _ in range(3):  # two eager warm-up steps in all, the capture, a replay
            trs[name].step()
        assert len(trs[name].graphs) == 1
    assert trs["bce"].prog.loss_kind == "bce" and trs["ce"].prog.loss_kind == "ce"
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
    per = window("ce", n) / n
    n = max(8, int(seconds / per + 7) // 8 * 8)
    readings = {"ce": [], "bce": []}
    for r in range(rounds):
        for slot, name in enumerate(("ce", "bce", "ce")):
            dt = window(name, n)
            rec = {"model": arch, "hw": hw, "batch": batch, "loss": name, "round": r, "slot": slot, "steps": n,
                   "ms_per_step": 1e3 * dt / n, "img_per_s": batch * n / dt}
            readings[name].append(rec["ms_per_step"])
            emit(rec, out)
    base, bce = readings["ce"], readings["bce"]
    m_base, m_bce = sum(base) / len(base), sum(bce) / len(bce)
    spread = max(abs(a - b) for a, b in zip(base[0::2], base[1::2]))
    emit({"summary": "steps", "model": arch, "hw": hw, "batch": batch, "classes": classes,
          "logits_bytes_read_and_written": 2 * batch * classes * 2,
          "ce_ms_per_step": m_base, "bce_ms_per_step": m_bce, "ce_spread_within_round_us": 1e3 * spread,
          "ce_spread_all_us": 1e3 * (max(base) - min(base)), "bce_minus_ce_us": 1e3 * (m_bce - m_base),
          "bce_minus_ce_us_per_round": [1e3 * (bce[r] - 0.5 * (base[2 * r] + base[2 * r + 1])) for r in range(rounds)],
          "predicted_us": 0.0, "prediction": "one launch-latency kernel replaces another: inside the ce spread",
          "bce_vs_ce": m_base / m_bce - 1.0}, out)
    trs.clear()
    import gc
    gc.collect()
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--models", default="resnet18:32:256,resnet50:224:1024", help="arch:image size:batch, ... ('' = none)")
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--seconds", type=float, default=1.0, help="least duration of one step reading")
    p.add_argument("--launches", type=int, default=200, help="kernel launches per captured graph")
    p.add_argument("--no-kernels", action="store_true", help="skip the kernels-alone readings")
    p.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = p.parse_args()
    if not torch.cuda.is_available():
        print("bench_bce: no GPU (a timing needs the device)", file=sys.stderr)
        sys.exit(2)
    out = open(a.out, "a") if a.out else None
    if not a.no_kernels:
        for B, C in KERNEL_SHAPES:
            bench_kernels(B, C, a.rounds, a.launches, out)
    for spec in filter(None, a.models.split(",")):
        arch, hw, batch = spec.split(":")
        bench_model(arch, int(hw), int(batch), a.rounds, a.seconds, out)
    if out is not None:
        out.close()


if __name__ == "__main__":
    main()
