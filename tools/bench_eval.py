#!/usr/bin/env python
"""Validation throughput on one GPU: the evaluation pass against the per-batch host path.

Both paths run in one process over the same resident synthetic batches, alternating round by round:

* ``host``: ``NativeTrainer.evaluate_batch`` (eager; weights and every BN's coefficients redone per
  batch) + torch's cross-entropy and argmax on the fp32 logits with two ``.item()`` per batch -- what
  ``train()`` does with ``eval_graph=false``;
* ``pass``: ``eval_begin`` once, one ``eval_step`` (a graph replay ending in ``ce_eval``) per batch,
  ``eval_end``'s one host read.

Every round is timed by the host clock around work that ends in a device synchronise. Reported per
shape: the median ms per batch of each path, their ratio, img/s next to the training step's, and both
paths' sums of the last round (``same_metrics``: equal counts, loss sums within twice the fp32 bound of
either, top-1 hits apart by no more than the rows whose largest logit is tied). One JSON line per shape
goes to ``--out``.

    python tools/bench_eval.py                     # ResNet-18 32x32 b256 and ResNet-50 224x224 b256
    python tools/bench_eval.py --shapes resnet18:32:10:256 --rounds 5 --batches 20
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

DEFAULT_SHAPES = ["resnet18:32:10:256", "resnet50:224:1000:256"]


def host_path(tr, data):
    loss, corr, n = 0.0, 0.0, 0
    for img, lab in data:
        logits = tr.evaluate_batch(img, lab).float()
        loss += F.cross_entropy(logits, lab, reduction="sum").item()
        corr += (logits.argmax(1) == lab).sum().item()
        n += lab.shape[0]
    return loss, corr, n


def pass_path(tr, data, topk):
    tr.eval_begin(topk=topk)
    for img, lab in data:
        tr.eval_step(img, lab)
    r = tr.eval_end()
    return r.loss_sum, r.top1, r.count


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def bench_shape(spec, args, dev):
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig
    from dbx_distributed_pytorch_examples_amd.models import build_model
    name, size, classes, batch = spec.split(":")
    size, classes, batch = int(size), int(classes), int(batch)
    torch.manual_seed(0)
    tr = NativeTrainer(build_model(name, num_classes=classes), batch, (size, size), dev, optim=OptimConfig(lr=0.01))
    g = torch.Generator().manual_seed(1)
    pool = [(torch.randint(0, 256, (batch, size, size, 3), dtype=torch.uint8, generator=g).to(dev),
             torch.randint(0, classes, (batch,), generator=g).to(dev)) for _ in range(4)]
    data = [pool[i % len(pool)] for i in range(args.batches)]
    # the training step (two eager steps, the capture, then replays) for the img/s beside
    for img, lab in data[:4]:
        tr.step(img, lab)
    t_train, _ = timed(lambda: [tr.step(img, lab) for img, lab in data], dev)
    tr.read_metrics()
    # warm both paths (the pass captures its graph on the third call)
    host_path(tr, data[:3])
    pass_path(tr, data[:4], args.topk)
    t_host, t_pass = [], []
    for _ in range(args.rounds):
        th, h = timed(lambda: host_path(tr, data), dev)
        tp, p = timed(lambda: pass_path(tr, data, args.topk), dev)
        t_host.append(th)
        t_pass.append(tp)
    # (untimed) rows whose largest logit is tied: there the pass counts a hit only for the lowest index, as
    # the training step does, while torch's argmax on the device may name any of the tied classes
    # and the plain fp32 bound of each path's loss sum against the exact one (tests/test_ce_eval.py): per row
    # 2^-20 (|lse| + |x_l|), plus the sum of a batch's fp32 terms; the two paths differ by at most twice that
    tied, mag = 0, 0.0
    for img, lab in data:
        lg = tr.evaluate_batch(img, lab).double()
        tied += int(((lg == lg.max(1, keepdim=True).values).sum(1) > 1).sum())
        mag += float((torch.logsumexp(lg, 1).abs() + lg.gather(1, lab[:, None]).squeeze(1).abs()).sum())
    loss_bound = 2 * (2.0 ** -20 * mag + (batch * 2.0 ** -24 + 2.0 ** -21) * max(abs(h[0]), abs(p[0])))
    same = h[2] == p[2] and abs(h[1] - p[1]) <= tied and abs(h[0] - p[0]) <= loss_bound
    nb = len(data)
    ms_host, ms_pass = (1e3 * statistics.median(t) / nb for t in (t_host, t_pass))
    rec = {"model": name, "image": size, "classes": classes, "batch": batch, "batches": nb, "rounds": args.rounds,
           "topk": args.topk, "host_ms_per_batch": ms_host, "pass_ms_per_batch": ms_pass,
           "pass_over_host": ms_pass / ms_host, "host_img_s": 1e3 * batch / ms_host,
           "pass_img_s": 1e3 * batch / ms_pass, "train_ms_per_step": 1e3 * t_train / nb,
           "train_img_s": batch * nb / t_train, "host_ms_rounds": [1e3 * t / nb for t in t_host],
           "pass_ms_rounds": [1e3 * t / nb for t in t_pass],
           "host_metrics": {"loss_sum": h[0], "top1": h[1], "count": h[2]},
           "pass_metrics": {"loss_sum": p[0], "top1": p[1], "count": p[2]}, "tied_max_rows": tied,
           "loss_sum_bound": loss_bound, "same_metrics": same,
           "device": torch.cuda.get_device_name(dev)}
    print(f"{name} {size}x{size} b{batch}: host {ms_host:.3f} ms/batch ({rec['host_img_s']:.0f} img/s), "
          f"pass {ms_pass:.3f} ms/batch ({rec['pass_img_s']:.0f} img/s), pass / host = {rec['pass_over_host']:.3f}; "
          f"training step {rec['train_ms_per_step']:.3f} ms ({rec['train_img_s']:.0f} img/s); "
          f"host / pass loss sum {h[0]:.6g} / {p[0]:.6g} (apart by {abs(h[0] - p[0]) / loss_bound:.3f} of the bound), top-1 {h[1]:.0f} / {p[1]:.0f} of {p[2]} "
          f"({tied} rows with a tied maximum); same metrics: {same}", flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", nargs="+", default=DEFAULT_SHAPES, help="model:image:classes:batch")
    ap.add_argument("--batches", type=int, default=40, help="batches per timed round")
    ap.add_argument("--rounds", type=int, default=7, help="alternations of the two paths")
    ap.add_argument("--topk", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "eval_graph", "bench_eval.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_eval.py measures on a GPU; none is visible")
    dev = torch.device("cuda", 0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for spec in args.shapes:
            f.write(json.dumps(bench_shape(spec, args, dev)) + "\n")
            f.flush()


if __name__ == "__main__":
    main()
