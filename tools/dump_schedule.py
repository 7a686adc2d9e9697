#!/usr/bin/env python
"""Record the training step's schedule as the constructors resolve it: one JSON row per engine spec,
step-size class and constructor.

For every spec the script builds ResNet-18 at 32x32, batch 2, with ``fwd_conv_flops`` patched to one
value per step-size class, through ``ResNetProgram``, ``NativeTrainer`` and ``NativeResNet`` (the
native module), and prints every schedule attribute it finds by name. It reads attributes with
``getattr`` only, so the same file runs on any commit; ``tests/golden/step_schedule.json`` is its
output on the commit before ``engine/schedule.py`` existed (CPU rows, and ``cuda`` rows from one
MI355X at world 1 with a process group), and ``tests/test_schedule_cpu.py`` holds
``resolve_schedule`` to every row of it.

    python tools/dump_schedule.py --device cpu  --out cpu.json
    python tools/dump_schedule.py --device cuda --out cuda.json
    python tools/dump_schedule.py --merge cpu.json cuda.json --out tests/golden/step_schedule.json

``--merge`` writes the fixture: one line per resolver input (spec, step-size class, context; the device is the
context's ``cuda``), the values in ``fields`` order, booleans as 0 / 1. Constructor runs that share an input (a ZeRO trainer and
a plain one, a program and a single-GPU trainer) must agree and fold into one line; "-" marks a field that
no constructor behind the line has (the trainer's, on a program-only line).
"""
import argparse
import itertools
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FLOPS = {"tiny": 1e10, "mid": 1e11, "large": 1e12}
PROGRAM_FIELDS = ("overlap_wgrad", "side_batch", "side_block", "side_block_default", "side_defer",
                  "side_cu_reserve", "stem_wg_main", "tail_main", "dwf_cus", "block_tail_main", "lazy_join",
                  "event_joins", "fold_min", "fold_max_ratio", "defer_reduce", "nshard", "fin_in", "coeff_in",
                  "coeff_in_maxc", "small_step")
TRAINER_FIELDS = ("block_posts", "late_posts", "comm_side", "separate_comm_stream")
CONTEXT = ("cuda", "segmented", "native_comm", "use_graphs", "in_order_wgrads")


def specs(device):
    """(spec, constructors, flop classes, trainer keywords): the single-GPU specs through all three
    constructors, the segmented cross through the trainer. The CPU has no communicator and no graphs, so
    its rows leave out ``comm=native`` and ``use_graphs=False``; ``cuda`` leaves out the single-GPU specs
    past the layouts (nothing device-dependent acts on them)."""
    cpu = device == "cpu"
    single = [""] + [f"overlap_wgrad={v}" for v in (0, 1, 2, 3)] + [
        "fuse_stem_bwd=1", "fuse_stem_bwd=1,overlap_wgrad=2", "fuse_stem_bwd=1,overlap_wgrad=3",
        "side_defer=0", "side_defer=1", "lazy_join=0", "lazy_join=1", "stem_wg_main=0", "stem_wg_main=1",
        "side_cu_reserve=64", "tail_main=0", "tail_main=2", "overlap_wgrad=2,side_defer=1", "block_tail_main=0",
        "dwf_cus=64", "nshard=8", "fin_in=1", "fin_in=0", "coeff_in=0", "coeff_in_maxc=0", "coeff_in_maxc=256",
        "defer_reduce=1", "fold_min_elems=4096", "fold_max_ratio=2.0", "overlap_wgrad=0,fold_min_elems=4096"]
    for i, s in enumerate(single if cpu else single[:8]):
        yield s, ("program",), tuple(FLOPS), {}
        if i < 8:
            yield s, ("trainer", "module", "module_world2"), ("mid",), {}
    yield "", ("trainer", "module", "module_world2"), ("tiny", "large"), {}
    cross = itertools.product(("native", "torch"), ("block", "batch"), (1, 0), (1, 0), (True, False))
    for comm, layout, comm_side, seg_side, graphs in cross:
        if cpu and (comm == "native" or not graphs):
            continue
        base = f"segmented_graphs=1,comm={comm},multirank_layout={layout},comm_side={comm_side},seg_side={seg_side}"
        yield base, ("trainer",), tuple(FLOPS), {"use_graphs": graphs}
        yield base + ",block_tail_main=0", ("trainer",), ("mid",), {"use_graphs": graphs}
        yield base, ("trainer",), ("mid",), {"use_graphs": graphs, "zero_stage": 1}
        yield base + ",block_tail_main=0", ("trainer",), ("mid",), {"use_graphs": graphs, "zero_stage": 1}
    extra = [f"overlap_wgrad={v}" for v in (0, 1, 2, 3)] + [
        "side_defer=0", "side_defer=1", "lazy_join=0", "lazy_join=1", "stem_wg_main=0", "stem_wg_main=1",
        "side_cu_reserve=32", "tail_main=2", "fuse_stem_bwd=1", "overlap_wgrad=2,seg_side=0",
        "multirank_layout=batch,lazy_join=1", "multirank_layout=batch,side_defer=0",
        "multirank_layout=batch,side_cu_reserve=32", "multirank_layout=batch,stem_wg_main=1"]
    for e in extra:
        if not cpu:
            yield f"segmented_graphs=1,comm=native,{e}", ("trainer",), tuple(FLOPS), {}
        yield f"segmented_graphs=1,comm=torch,{e}", ("trainer",), ("mid",), {}


def read(obj, names):
    return {n: getattr(obj, n) for n in names if hasattr(obj, n)}


def build(kind, spec, dev, kw):
    """One constructor run; returns (context facts the schedule depends on, schedule values)."""
    import torch
    import torch.distributed as dist
    from dbx_distributed_pytorch_examples_amd.engine.native_module import NativeResNet
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer
    from dbx_distributed_pytorch_examples_amd.engine.program import ResNetProgram
    from dbx_distributed_pytorch_examples_amd.models import build_model
    os.environ["DBX_ENGINE"] = spec
    model = build_model("resnet18", num_classes=10)
    ctx = {"cuda": dev.type == "cuda", "segmented": False, "native_comm": False, "use_graphs": False,
           "in_order_wgrads": False}
    if kind == "program":
        return ctx, read(ResNetProgram(model, 2, (32, 32), dev), PROGRAM_FIELDS)
    if kind == "trainer":
        if "segmented_graphs=1" in spec and not dist.is_initialized():
            dist.init_process_group("gloo", init_method=f"file://{tempfile.mkdtemp()}/pg", rank=0, world_size=1)
        t = NativeTrainer(model, 2, (32, 32), dev, **kw)
        ctx.update(segmented=bool(t.segmented), native_comm=t.ncomm is not None, use_graphs=bool(t.use_graphs))
        vals = {**read(t.prog, PROGRAM_FIELDS), **read(t, TRAINER_FIELDS)}
        vals["separate_comm_stream"] = t.comm_stream is not None and t.comm_stream is not t.prog._wstream
        if t.ncomm is not None:
            t.ncomm.close()
        return ctx, vals
    m = NativeResNet(model, None, None, dev)
    if kind == "module_world2":  # what _build does for a world > 1, without the second rank
        m.world = 2
        ctx["in_order_wgrads"] = True
    m._build(2, (32, 32))
    return ctx, read(m.prog, PROGRAM_FIELDS)


def fold(rows):
    """The fixture's lines: recorded rows that the current spec list asks for, one per resolver input."""
    want = {(d, spec, FLOPS[c], k, json.dumps(kw, sort_keys=True)) for d in ("cpu", "cuda")
            for spec, kinds, classes, kw in specs(d) for k in kinds for c in classes}
    fields = PROGRAM_FIELDS + TRAINER_FIELDS
    out = {}
    for r in rows:
        if (r["device"], r["spec"], r["flops"], r["constructor"], json.dumps(r["kw"], sort_keys=True)) not in want:
            continue
        key = (r["spec"], r["flops"], "+".join(c for c in CONTEXT if r["ctx"][c]))
        line = out.setdefault(key, {})
        for f, v in r["schedule"].items():
            assert line.setdefault(f, v) == v, (key, f, line[f], v)
    cls = {v: k for k, v in FLOPS.items()}
    return fields, [[spec, cls[fl], ctx, [int(v) if isinstance(v, bool) else v for v in (line.get(f, "-") for f in fields)]]
                    for (spec, fl, ctx), line in out.items()]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", default="cpu", choices=["cpu", "cuda"])
    ap.add_argument("--out", required=True)
    ap.add_argument("--merge", nargs="+", help="recorded row files to fold into the fixture instead of recording")
    a = ap.parse_args()
    if a.merge:
        fields, lines = fold([r for f in a.merge for r in json.load(open(f))])
        with open(a.out, "w") as f:
            f.write('{"fields": %s,\n "context": %s,\n "flops": %s,\n "rows": [\n'
                    % (json.dumps(fields), json.dumps(CONTEXT), json.dumps(FLOPS)))
            f.write(",\n".join(json.dumps(l) for l in lines) + "\n]}\n")
        print(f"[dump_schedule] {len(lines)} lines -> {a.out}")
        return
    import torch
    from dbx_distributed_pytorch_examples_amd.engine.program import ResNetProgram
    dev, rows = torch.device(a.device), []
    for spec, kinds, classes, kw in specs(a.device):
        for kind, cls in itertools.product(kinds, classes):
            ResNetProgram.fwd_conv_flops = lambda self, f=FLOPS[cls]: f
            ctx, vals = build(kind, spec, dev, kw)
            rows.append({"spec": spec, "flops": FLOPS[cls], "constructor": kind, "kw": kw,
                         "device": a.device, "ctx": ctx, "schedule": vals})
            if len(rows) % 50 == 0:
                print(f"[dump_schedule] {len(rows)} rows", flush=True)
    json.dump(rows, open(a.out, "w"))
    print(f"[dump_schedule] {len(rows)} rows -> {a.out}")


if __name__ == "__main__":
    main()
