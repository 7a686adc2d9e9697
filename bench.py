#!/usr/bin/env python3
"""Headline benchmark: ResNet-50 ImageNet-1K (224x224, 1000 classes) training throughput.

Metric (BASELINE.json): images/sec for the whole job, ResNet-50 ImageNet-1K, at 1/2/4/8
MI355X, bf16, synthetic data + random-init weights, weak scaling (fixed per-GPU batch).

  python bench.py --gpus N --steps K --warmup W        # N=1 runs in-process; N>1 spawns N ranks itself
  python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...

With ``--gpus N > 1`` and no launcher environment (no WORLD_SIZE), bench.py starts N local rank
processes itself (the reference's ``TorchDistributor(num_processes=N, local_mode=True).run(...)``,
`01_torch_distributor/01_basic_torch_distributor.py:360-367`) before anything touches the GPU, and
exits with the worst rank's exit code. Under torchrun / our launcher it runs as the given rank. A
world size that differs from ``--gpus`` is an error (exit 3), and the JSON line reports the world
size the process group actually formed (``world_size_seen``) and its backend.

Implementations (``--impl``):
  native  the framework's flagship path: NHWC bf16 ResNet program on the hand-written HIP
          kernels (dbx.ops), graph-captured step, flat-bucket DDP on RCCL (default)
  torch   reference-equivalent stock PyTorch-ROCm: eager nn.Module, autocast bf16,
          torch DDP on RCCL, torch.optim.SGD — the measured "reference" column of BASELINE.md

Every timed step does the full work: input normalisation from uint8, forward, loss,
backward, gradient all-reduce (N>1) and the SGD-momentum update.

A plain run sets up, warms up, times ``--steps`` steps and prints one JSON line (``ms_per_step`` is
the time of one timed step). ``--dump-outputs DIR`` then writes what the last timed step computed
as ``DIR/<name>.npy`` so that two builds can be compared output for output (the inputs and the
initial weights are seeded: identical from run to run). ``--full`` is where secondary
measurements belong; there are none today.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dbx_distributed_pytorch_examples_amd  # noqa: E402,F401  (runtime settings read at HIP init)

# Reference-equivalent stock PyTorch ResNet-50 throughput on ONE MI355X, measured with
# `python bench.py --impl torch --batch B` (eager nn.Module, channels_last, autocast bf16, MIOpen
# convs, torch.optim.SGD; BASELINE.md, profiles/r1_torch_reference/). Keyed by per-GPU batch.
BASELINE_IMG_PER_SEC_PER_GPU = {256: 5941.96, 1024: 6496.62}
# ... and for BASELINE.json's other configs (same measurement method)
PRESET_BASELINE_PER_GPU = {"resnet18_cifar10": 52051.0, "resnet50_tiny_imagenet": 17714.0,
                           "resnet50_imagenet_zero1": 5970.0}
HEADLINE_METRIC = "images/sec (whole node) ResNet-50 ImageNet-1K at 1/2/4/8 MI355X; top-1 acc"
PRESET_METRIC = {
    "resnet18_cifar10": "images/sec (whole node) ResNet-18 CIFAR-10 32x32 DDP bf16 (BASELINE.json config 2)",
    "resnet50_tiny_imagenet": "images/sec (whole node) ResNet-50 TinyImageNet 64x64 DDP bf16 (BASELINE.json config 3)",
    "resnet50_imagenet_zero1": "images/sec (whole node) ResNet-50 ImageNet-1K ZeRO-1 AdamW bf16 (BASELINE.json config 4)",
    "resnet50_imagenet_8192": HEADLINE_METRIC,
}
DATASET_NAME = {(32, 10): "CIFAR-10", (64, 200): "TinyImageNet-200", (224, 1000): "ImageNet-1K"}

# BASELINE.json's other configs (the headline default is ResNet-50 ImageNet-1K, 1024/GPU).
PRESETS = {
    "resnet18_cifar10": dict(model="resnet18", image_size=32, num_classes=10, batch=256),
    "resnet50_tiny_imagenet": dict(model="resnet50", image_size=64, num_classes=200, batch=512),
    "resnet50_imagenet_zero1": dict(model="resnet50", image_size=224, num_classes=1000, batch=256, optim="adamw",
                                    zero=1),
    "resnet50_imagenet_8192": dict(model="resnet50", image_size=224, num_classes=1000, batch=1024),
}


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--batch", type=int, default=1024,
                   help="per-GPU batch (weak scaling); 1024 x 8 GPUs = the 8192 large-batch north-star config")
    p.add_argument("--impl", default="native", choices=["native", "torch"])
    p.add_argument("--model", default="resnet50")
    p.add_argument("--image-size", type=int, default=224)
    p.add_argument("--num-classes", type=int, default=1000)
    p.add_argument("--channels-last", type=int, default=1, help="torch impl only")
    p.add_argument("--lr", type=float, default=None, help="default: 0.1 (sgd) / 2e-4 (adamw)")
    p.add_argument("--optim", default="sgd", choices=["sgd", "adamw", "lars"])
    p.add_argument("--zero", type=int, default=0, choices=[0, 1, 2], help="native impl: ZeRO stage")
    p.add_argument("--preset", default="", choices=[""] + sorted(PRESETS),
                   help="one of BASELINE.json's other configs (sets model/size/classes/batch/optim)")
    p.add_argument("--data", default="synthetic", choices=["synthetic", "mds"],
                   help="mds: every step's batch comes from zstd MDS shards written first (the 03a path): "
                        "C++ shard reader -> pinned staging ring -> async H2D -> GPU augment -> native step")
    p.add_argument("--mds-samples", type=int, default=0, help="samples per rank written for --data mds "
                   "(default: enough for warmup + steps, at least 8 batches)")
    p.add_argument("--json-out", default=None)
    p.add_argument("--dump-outputs", default=None, metavar="DIR",
                   help="after the timed steps, write what the last step left for its caller (logits, the metric "
                        "accumulators, parameters, gradients) as DIR/<name>.npy, float32 / float64, at most 64 MB "
                        "(large arrays: a fixed seeded sample); same arguments -> same inputs, run to run")
    p.add_argument("--full", action="store_true",
                   help="also run the benchmark's secondary measurements; a plain run does only what the headline "
                        "figure needs (set up, warm up, time --steps steps). Nothing is secondary today: every "
                        "other measurement is a run of its own (--impl torch, --preset, --data mds, --gpus N)")
    p.add_argument("--phase-timeout", type=float, default=300.0,
                   help="world > 1: watchdog bound (s) on every phase (setup / warm-up / timed / checks); exit 75")
    p.add_argument("--comm-fallback", type=int, default=1, choices=[0, 1],
                   help="world > 1: re-run failed ranks once, fresh, on the c10d step (comm=torch)")
    p.add_argument("--rccl-summary", type=int, default=1, choices=[0, 1],
                   help="world > 1 on RCCL: log RCCL's rings / channels to a file and summarise them in the JSON")
    a = p.parse_args(argv)
    given = {t.split("=", 1)[0] for t in (sys.argv[1:] if argv is None else argv) if t.startswith("--")}
    for k, v in PRESETS.get(a.preset, {}).items():
        if "--" + k.replace("_", "-") not in given:  # explicit flags win over the preset's values
            setattr(a, k, v)
    if a.lr is None:
        a.lr = {"sgd": 0.1, "lars": 9.0}.get(a.optim, 2e-4)
    return a


def self_launch(args, argv) -> int:
    """Spawn ``args.gpus`` local ranks of this script (no GPU call happens in this process first:
    torch.cuda.device_count() does not initialise HIP)."""
    backend = os.environ.get("DBX_DIST_BACKEND", "")
    ndev = torch.cuda.device_count()
    if backend != "gloo" and ndev < args.gpus:
        print(f"[bench] error: --gpus {args.gpus} but {ndev} GPU(s) visible (RCCL needs one GPU per rank; "
              f"DBX_DIST_BACKEND=gloo rehearses several ranks on one device)", file=sys.stderr)
        return 3
    from dbx_distributed_pytorch_examples_amd.launch import describe_exit, run_subprocess_ranks
    cmd = [sys.executable, os.path.abspath(__file__)] + list(argv)
    rc = run_subprocess_ranks(args.gpus, cmd)
    if rc == 0 or not _may_fall_back(args) or not _retryable(rc):
        return rc
    # the ranks failed on the default (framework-RCCL one-graph) step -- e.g. a hung collective ended by
    # the watchdog (75): this parent never touched the GPU, so it starts FRESH ranks once on the c10d step
    reason = f"attempt 1 failed: worst rank {describe_exit(rc)}"
    print(f"[bench] {reason}; re-running {args.gpus} fresh ranks with comm=torch", file=sys.stderr, flush=True)
    return run_subprocess_ranks(args.gpus, cmd, env={**fallback_env(reason), "DBX_RESTART_COUNT": "1"})


def _engine():
    from dbx_distributed_pytorch_examples_amd.engine_config import EngineConfig
    return EngineConfig.current()


def _may_fall_back(args) -> bool:
    """A failed multi-rank native run is re-measured once on fresh ranks (c10d collectives) unless it
    already is that re-measurement, runs on c10d anyway, or --comm-fallback 0."""
    return (args.impl == "native" and args.comm_fallback == 1 and not os.environ.get("DBX_BENCH_RETRY")
            and _engine().comm != "torch")


def _retryable(rc: int) -> bool:
    # 2 = usage error, 3 = world / --gpus mismatch, 4 = replicas diverged on the c10d path too: a re-run
    # would repeat them. Anything else (watchdog 75, abort, segfault, a raised error) may be the one-graph
    # RCCL step's own failure.
    return rc not in (0, 2, 3, 4)


def fallback_env(reason: str) -> dict:
    from dbx_distributed_pytorch_examples_amd.engine_config import engine_env
    return {"DBX_ENGINE": engine_env(comm="torch"), "DBX_BENCH_RETRY": reason}


def supervise(args, argv) -> int:
    """Under torchrun (the driver's N-GPU command): this rank process becomes a GPU-free supervisor of a
    child that does the work, so a failed one-graph attempt can be re-run on fresh ranks
    (``launch.supervise_rank``)."""
    from dbx_distributed_pytorch_examples_amd.launch import supervise_rank
    return supervise_rank([sys.executable, os.path.abspath(__file__)] + list(argv), fallback_env, _retryable)


def _rccl_log_setup(info_world: int, on: bool = True) -> str:
    """World > 1 on RCCL: route RCCL's INFO log (rings, channels, version) to a per-process file unless the
    user set NCCL_DEBUG (then it passes through untouched). Returns the file path ('' = none)."""
    if info_world <= 1 or os.environ.get("DBX_DIST_BACKEND") == "gloo" or not on:
        return ""
    if "NCCL_DEBUG" in os.environ:
        return os.environ.get("NCCL_DEBUG_FILE", "")
    import tempfile
    path = os.path.join(tempfile.gettempdir(), f"dbx_rccl_{os.getpid()}.log")
    os.environ["NCCL_DEBUG"] = "INFO"
    os.environ["NCCL_DEBUG_FILE"] = path
    return path


def rccl_summary(path: str) -> dict:
    """Version, channel count and the first ring(s) from an RCCL INFO log."""
    import re
    import socket
    if not path:
        return {}
    path = path.replace("%h", socket.gethostname()).replace("%p", str(os.getpid()))
    try:
        with open(path, errors="replace") as f:
            lines = f.read().splitlines()
    except OSError:
        return {}
    out: dict = {}
    rings, nch = [], 0
    for ln in lines:
        m = re.search(r"(RCCL|NCCL) version\s*(\S+)", ln)
        if m and "version" not in out:
            out["version"] = m.group(2)
        m = re.search(r"Channel (\d+)/(\d+) :((?:\s+\d+)+)\s*$", ln)
        if m:
            nch = max(nch, int(m.group(2)))
            if len(rings) < 2:
                rings.append(" ".join(m.group(3).split()))
        m = re.search(r"(\d+) coll channels", ln)
        if m:
            out["coll_channels"] = int(m.group(1))
    if nch:
        out["channels"] = nch
        out["rings"] = rings
    out["log_lines"] = len(lines)
    if os.environ.get("NCCL_DEBUG_FILE", "").startswith(os.path.join(os.path.dirname(path), "dbx_rccl_")):
        try:
            os.remove(path)
        except OSError:
            pass
    return out


def replicas_in_sync(step, info, when: str, wd=None) -> bool:
    """World > 1: every rank must hold bit-identical parameters after data-parallel steps (the DP
    fp32 master, or ZeRO's all-gathered bf16 copy; the torch impl: the module's parameters). A
    mis-ordered or mis-summed collective then fails the run instead of printing a number."""
    if info.world_size == 1:
        return True
    from dbx_distributed_pytorch_examples_amd.utils.debug import assert_replicas_in_sync
    tensors = _replica_tensors(step)
    if wd is not None:
        wd.step_begin(f"replica check after {when}")
    try:
        assert_replicas_in_sync(tensors, rtol=0.0, what=f"parameters after {when}")
    except AssertionError as e:
        print(f"[bench] error: {e}; refusing to report a number", file=sys.stderr, flush=True)
        return False
    finally:
        if wd is not None:
            wd.step_end()
    if info.rank == 0:
        print(f"[bench] replicas in sync after {when} ({info.world_size} ranks, bit-identical parameters)",
              file=sys.stderr, flush=True)
    return True


def _replica_tensors(step):
    tr = getattr(step, "trainer", None)
    if tr is not None:
        return [tr.zero.param16] if tr.zero is not None else [tr.prog.master]
    return [p.detach() for p in getattr(step, "model").parameters()]


DUMP_MAX_ELEMS = 3 << 20  # per array: 12 MiB of float32, so the four arrays of a step stay under 64 MB
DUMP_SAMPLE_SEED = 20240611


def step_outputs(step) -> dict:
    """What the last step left for its caller, by name. Native: the head's logits of the last batch, the
    metric accumulators (loss sum and correct count over every step since set-up), the flat fp32
    parameters after the update and, without ZeRO, the flat gradient that update used (under ZeRO a
    rank only holds its reduced shard). Torch impl: logits, loss, parameters, gradients."""
    tr = getattr(step, "trainer", None)
    if tr is not None:
        tr.sync_master()  # ZeRO: every rank's shard of the master (collective; a no-op otherwise)
        out = {"logits": tr.prog.logits, "loss_sum_correct": tr.prog.metrics[:2], "params": tr.prog.master}
        if tr.zero is None:
            out["grads"] = tr.prog.grad
        return out
    ps = [p for p in step.model.parameters()]
    return {"logits": step.logits, "loss": step.loss.reshape(1),
            "params": torch.cat([p.detach().reshape(-1) for p in ps]),
            "grads": torch.cat([p.grad.reshape(-1) for p in ps if p.grad is not None])}


def dump_outputs(step, info, out_dir: str) -> None:
    """``--dump-outputs``: rank 0 writes ``step_outputs`` as ``<out_dir>/<name>.npy`` (float64 stays
    float64, everything else becomes float32). An array of more than ``DUMP_MAX_ELEMS`` elements is
    sampled at fixed positions (sorted draws of a seeded generator, the same for every run and build)."""
    import numpy as np
    outs = step_outputs(step)  # on every rank: may hold a collective
    if info.device.type == "cuda":
        torch.cuda.synchronize()
    if info.rank != 0:
        return
    os.makedirs(out_dir, exist_ok=True)
    for name, t in outs.items():
        t = t.detach()
        if t.numel() > DUMP_MAX_ELEMS:
            t = t.reshape(-1)
            rng = np.random.default_rng(DUMP_SAMPLE_SEED)
            idx = np.sort(rng.integers(0, t.numel(), size=DUMP_MAX_ELEMS, dtype=np.int64))
            t = t[torch.from_numpy(idx).to(t.device)]
        a = t.to(torch.float64 if t.dtype == torch.float64 else torch.float32).cpu().numpy()
        np.save(os.path.join(out_dir, name + ".npy"), a)


def _measure(args, info, wd, build_step, ddist, fault):
    """Build the step, warm up, check the replicas, time ``args.steps`` steps, check again.
    Returns (rc, elapsed seconds (max over ranks), meta); rc 4 = replicas diverged."""
    step, meta = build_step(args, info)
    tr = getattr(step, "trainer", None)
    meta["_native_comm"] = getattr(tr, "ncomm", None) is not None
    if wd is not None:
        wd.register(getattr(tr, "ncomm", None))
        wd.step_end()

    def sync():
        if info.device.type == "cuda":
            torch.cuda.synchronize()

    def release():  # a rebuilt step must not hold the first one's buffers / graphs / communicator
        nonlocal step, tr
        if tr is not None and getattr(tr, "ncomm", None) is not None:
            if wd is not None:
                wd.unregister(tr.ncomm)  # (the watchdog polls registered communicators)
            tr.ncomm.close()
        step = tr = None
        import gc
        gc.collect()
        if info.device.type == "cuda":
            torch.cuda.empty_cache()

    inject = fault.parse_fault() is not None  # DBX_FAULT=rank:step:kind (warm-up steps only)
    if wd is not None:
        wd.step_begin("warmup")
    for i in range(args.warmup):
        if inject:
            fault.maybe_inject(i)
        step()
    sync()
    ddist.barrier()
    sync()
    if wd is not None:
        wd.step_end()
    spec = fault.parse_fault()
    if spec is not None and spec[2] == "diverge" and spec[0] == info.rank:
        _replica_tensors(step)[0].view(-1)[:1].add_(1.0)  # injected divergence (tests the replica check)
    if not replicas_in_sync(step, info, "warm-up", wd):
        release()
        return 4, 0.0, meta
    if wd is not None:
        wd.step_begin("timed")
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    sync()
    ddist.barrier()
    sync()
    elapsed = time.perf_counter() - t0
    elapsed = ddist.all_reduce_max(elapsed)
    if wd is not None:
        wd.step_end()
    if not replicas_in_sync(step, info, "the timed steps", wd):
        release()
        return 4, 0.0, meta
    if args.dump_outputs:
        dump_outputs(step, info, args.dump_outputs)
    return 0, elapsed, meta


def main(argv=None) -> int:
    raw = list(sys.argv[1:] if argv is None else argv)
    args = parse_args(raw)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return self_launch(args, raw)
    if (args.gpus > 1 and not os.environ.get("DBX_SUPERVISED_CHILD") and _may_fall_back(args)
            and os.environ.get("TORCHELASTIC_USE_AGENT_STORE") == "True"):
        return supervise(args, raw)
    rccl_log = _rccl_log_setup(int(os.environ.get("WORLD_SIZE", "1")), args.rccl_summary == 1)
    from dbx_distributed_pytorch_examples_amd.parallel import dist as ddist
    from dbx_distributed_pytorch_examples_amd.train.bench_steps import build_step

    info = ddist.init_distributed()
    import torch.distributed as tdist
    seen = tdist.get_world_size() if tdist.is_initialized() else 1
    if seen != args.gpus or info.world_size != args.gpus:
        print(f"[bench] error: --gpus {args.gpus} but the process group has {seen} rank(s) "
              f"(WORLD_SIZE={info.world_size}); refusing to report a mislabelled number", file=sys.stderr)
        ddist.destroy()
        return 3
    torch.manual_seed(1234 + info.rank)
    # world > 1: a watchdog bounds every phase (a hung collective or rank ends the job with the phase
    # and rank named, exit 75, instead of blocking until the driver's timeout); it brackets whole
    # phases, so nothing is added inside the timed loop
    wd = None
    if info.world_size > 1:
        from dbx_distributed_pytorch_examples_amd.parallel.comm_guard import CommWatchdog
        wd = CommWatchdog(timeout_s=args.phase_timeout, device=info.device)
    from dbx_distributed_pytorch_examples_amd.utils import fault
    comm_fallback = os.environ.get("DBX_BENCH_RETRY") or None
    for attempt in (0, 1):
        if wd is not None:
            wd.step_begin("setup")
        rc, elapsed, meta = _measure(args, info, wd, build_step, ddist, fault)
        # the one-graph multi-rank step (framework RCCL communicator) is checked here against its own
        # replicas: if they diverged, every rank saw it (the check gathers all checksums) and all of them
        # rebuild the step on the c10d path (comm=torch) and measure again instead of failing
        if rc == 4 and attempt == 0 and meta.get("_native_comm"):
            if info.rank == 0:
                print("[bench] warning: the one-graph step's replicas diverged; re-measuring on the c10d "
                      "collectives (comm=torch)", file=sys.stderr, flush=True)
            from dbx_distributed_pytorch_examples_amd.engine_config import engine_env
            os.environ["DBX_ENGINE"] = engine_env(comm="torch")
            comm_fallback = "replicas_diverged on the one-graph step; re-measured in-process with comm=torch"
            continue
        break
    if rc != 0:
        return rc
    meta.pop("_native_comm", None)
    if wd is not None:
        wd.close()

    n = info.world_size
    imgs = args.batch * n * args.steps
    value = imgs / elapsed
    headline = (args.model == "resnet50" and args.image_size == 224 and args.num_classes == 1000
                and args.optim == "sgd" and not args.zero)
    if headline:
        base = BASELINE_IMG_PER_SEC_PER_GPU.get(args.batch)
    elif args.preset in PRESET_BASELINE_PER_GPU and args.batch == PRESETS[args.preset]["batch"]:
        base = PRESET_BASELINE_PER_GPU[args.preset]
    else:
        base = None
    metric = PRESET_METRIC.get(args.preset, HEADLINE_METRIC) if (args.preset or headline) else (
        f"images/sec (whole node) {args.model} {args.image_size}x{args.image_size} {args.num_classes}-class bf16")
    dname = DATASET_NAME.get((args.image_size, args.num_classes), f"{args.num_classes}-class")
    out = {
        "metric": metric,
        "value": round(value, 2),
        "unit": "images/s",
        "n_gpus": n,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(1000.0 * elapsed / args.steps, 3),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": (round(value / (base * n), 4) if base else None),
        "dtype": "bf16",
        **({"comm_fallback": comm_fallback} if n > 1 else {}),
        "data": (f"synthetic (uint8 NHWC {args.image_size}x{args.image_size} images + random labels, on-device; "
                 "random-init weights)") if args.data == "synthetic" else (
            f"synthetic images of the config's shape streamed from zstd MDS shards ({meta.get('mds', '')}); "
            "random-init weights"),
        "config": {
            "model": f"{args.model} {dname} {args.image_size}x{args.image_size} {args.num_classes} classes"
                     + (" large-batch (global 8192 at 8 GPUs)" if headline and args.batch == 1024 else ""),
            "global_batch": args.batch * n,
            "per_gpu_batch": args.batch,
            "seq_len": None,
            "parallelism": f"dp{n}" + (f"+zero{args.zero}" if args.zero else ""),
            "world_size_seen": seen,
            "backend": info.backend,  # "none" without a process group (a world-1 run unless DBX_FORCE_PG=1)
            "impl": args.impl,
            "optimizer": {"sgd": "SGD momentum 0.9 nesterov=False wd 5e-5",
                          "lars": "LARS (eta 1e-3) + SGD momentum 0.9 wd 5e-5"}.get(args.optim, "AdamW wd 0.01")
                         + (f", ZeRO-{args.zero}" if args.zero else ""),
            **meta,
        },
    }
    if n > 1:
        rs = rccl_summary(rccl_log) if info.rank == 0 else {}
        if rs:
            out["config"]["rccl"] = rs
    if info.rank == 0:
        line = json.dumps(out)
        print(line, flush=True)
        if args.json_out:
            with open(args.json_out, "w") as f:
                f.write(line + "\n")
    ddist.destroy()
    return 0


if __name__ == "__main__":
    sys.exit(main())
