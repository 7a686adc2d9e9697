"""ZeRO-1 / ZeRO-2 sharded optimizers over flat fp32 buffers.

The reference ships DeepSpeed ZeRO configs (`/root/reference/02_deepspeed/deepspeed_config.py:53-105`:
stage 1 with ``overlap_comm``, ``contiguous_gradients``, ``reduce_scatter`` and 5e8 buckets; stage
2; stage 3; stage 3 + CPU offload) but never passes them to DeepSpeed. Here
they are real, with DeepSpeed's communication pattern:

* :class:`SegmentedZero` (the native ResNet program, ``NativeTrainer(zero_stage=1|2)``):
  - each backward segment's gradient range (head | layer4 | layer3 | layer2 | layer1 | stem,
    padded so it splits into ``world`` equal parts) is **reduce-scattered** on the comm stream
    as soon as that segment's backward graph has run, overlapped with the remaining backward
    (``overlap_comm`` + ``reduce_scatter``); rank r receives the summed gradient of part r of
    every segment -- its shard;
  - the fused AdamW / SGD kernel updates only the shard of the fp32 master with the
    shard-sized optimizer state, and writes the updated shard as **bf16** into a staging buffer;
  - one **bf16 all-gather** per segment rebuilds the full bf16 parameter copy (``prog.param16``)
    the next forward's weight preparation reads; the fp32 BatchNorm affine parameters (consumed
    in fp32 by the BN kernels) are exchanged exactly in fp32 (~0.2 % of the parameters).

  Per step each rank sends (w-1)/w x (4 + 2) bytes per parameter (fp32 reduce-scatter + bf16
  all-gather) instead of 2 (w-1)/w x 4 for a data-parallel all-reduce followed by an fp32
  parameter all-gather. No collective is captured: the update runs inside the step's HIP graph
  at any world size, the collectives are issued between graph replays. Stages 1 and 2 have the
  same traffic here (the program's flat gradient buffer is resident either way; ResNet-50's
  102 MB of fp32 gradients are nothing against 288 GB of HBM).
* :class:`ZeroShardedOptimizer` (generic flat buffers, the autograd engine): stage 1 slices the
  already all-reduced gradient, stage 2 reduce-scatters it; same shard update + all-gather.

Both are bit-compatible with plain data parallel + the same optimizer (tests/test_dist_cpu.py,
tools/dist_gpu_check.py). Stage 3 (parameter sharding) and CPU offload live in ``parallel/fsdp.py``.
"""
from __future__ import annotations

import math
import os
import warnings
from typing import List, Optional, Tuple

import torch
import torch.distributed as dist

from ..ops import kernels as K
from ..config import reject_param_groups
from .dist import host_sync_for_gloo


def shard_range(n: int, rank: int, world: int, align: int = 16) -> Tuple[int, int]:
    """Contiguous, 16-element aligned shard [lo, hi) of an n-element flat buffer."""
    per = (n + world - 1) // world
    per = (per + align - 1) // align * align
    lo = min(n, rank * per)
    return lo, min(n, lo + per)


class ZeroShardedOptimizer:
    """Optimizer step over a flat master buffer with sharded optimizer state.

    ``master`` / ``grad``: fp32 flat tensors (same length; the DDP/native trainers' buffers).
    ``optim``: object with fields name, lr, momentum, nesterov, weight_decay, betas, eps, grad_clip.
    ``grads_already_reduced``: stage 1 with grads all-reduced (summed) by the caller's buckets.
    """

    def __init__(self, master: torch.Tensor, grad: torch.Tensor, optim, stage: int = 1, process_group=None,
                 grad_scale: Optional[float] = None):
        if stage not in (1, 2, 3):
            raise ValueError("ZeRO stage must be 1, 2 or 3")
        if optim.name not in ("sgd", "adam", "adamw"):
            raise ValueError(f"sharded optimizer supports sgd / adam / adamw, not {optim.name!r}")
        K.reject_dampening(optim)
        reject_param_groups(optim, "the sharded (ZeRO) optimizer")
        if stage == 3:
            warnings.warn("flat-buffer ZeRO: stage 3 runs as stage 2 here; parameter sharding is parallel.fsdp.ShardedDataParallel")
            stage = 2
        self.stage = stage
        self.master, self.grad, self.o = master, grad, optim
        self.pg = process_group
        self.world = dist.get_world_size(process_group) if dist.is_available() and dist.is_initialized() else 1
        self.rank = dist.get_rank(process_group) if self.world > 1 else 0
        n = master.numel()
        # pad the flat length to world * shard so all-gather / reduce-scatter see equal shards
        per = shard_range(n, 0, self.world)[1]
        self.per = per
        self.padded = per * self.world
        self.lo, self.hi = self.rank * per, min(n, (self.rank + 1) * per)
        dev = master.device
        self.m = torch.zeros(per, device=dev)
        self.v = torch.zeros(per, device=dev) if optim.name in ("adam", "adamw") else None
        self.step_count = 0
        self.grad_scale = grad_scale if grad_scale is not None else 1.0 / self.world
        self._gshard = torch.zeros(per, device=dev)
        self._pshard = torch.zeros(per, device=dev)
        self._clip = torch.zeros(4, device=dev)
        # padded full-length staging (reduce-scatter input / all-gather output): allocated once
        self._full = torch.zeros(self.padded, device=dev) if (self.world > 1 and self.padded != n) else None

    def shard_of(self, t: torch.Tensor) -> torch.Tensor:
        return t[self.lo:self.hi]

    def _padded_view(self, t: torch.Tensor) -> torch.Tensor:
        if t.numel() == self.padded:
            return t
        self._full[:t.numel()].copy_(t)  # the pad tail stays zero
        return self._full

    @torch.no_grad()
    def step(self, grads_already_reduced: bool = True, lr: Optional[float] = None,
             hyper: Optional[torch.Tensor] = None):
        """``hyper``: optional fp32 device tensor (lr, 1-b1^t, 1-b2^t) read by the kernels at run
        time. The native trainer passes its own so a graph-captured step follows LR schedules and
        Adam bias correction on every replay (host scalars would be frozen at capture)."""
        o = self.o
        self.step_count += 1
        n_own = self.hi - self.lo
        g = self._gshard
        g.zero_()
        if self.world > 1:
            host_sync_for_gloo(self.grad, self.pg)
        if self.world == 1:
            g[:n_own].copy_(self.grad[self.lo:self.hi])
        elif self.stage == 1 or grads_already_reduced:
            if not grads_already_reduced:
                dist.all_reduce(self.grad, group=self.pg)
            g[:n_own].copy_(self.grad[self.lo:self.hi])
        else:
            full = self._padded_view(self.grad)
            try:
                dist.reduce_scatter_tensor(g, full, group=self.pg)
            except (RuntimeError, NotImplementedError, AttributeError):
                dist.all_reduce(full, group=self.pg)
                g.copy_(full[self.rank * self.per:(self.rank + 1) * self.per])
        p = self._pshard
        p.zero_()
        p[:n_own].copy_(self.master[self.lo:self.hi])
        gsp = None
        if getattr(o, "grad_clip", 0.0):
            # global norm over all shards: local sum of squares, all-reduced
            local = (g[:n_own] * self.grad_scale).float().pow(2).sum()
            if self.world > 1:
                host_sync_for_gloo(local, self.pg)
                dist.all_reduce(local, group=self.pg)
            self._clip[2] = torch.clamp(o.grad_clip / (local.sqrt() + 1e-6), max=1.0)
            gsp = self._clip[2:3]
        lr = o.lr if lr is None else lr
        K.optim_step(o, p, g, self.m, self.v, None, step=self.step_count, lr=lr, grad_scale_ptr=gsp,
                     grad_scale=self.grad_scale, hyper=hyper)
        if self.world == 1:
            self.master[self.lo:self.hi].copy_(p[:n_own])
            return
        full = self.master if self._full is None else self._full
        host_sync_for_gloo(p, self.pg)
        dist.all_gather_into_tensor(full, p, group=self.pg)
        if full is not self.master:
            self.master.copy_(full[:self.master.numel()])

    def state_dict(self):
        return {"stage": self.stage, "step": self.step_count, "rank": self.rank, "world": self.world,
                "m": self.m.cpu(), "v": None if self.v is None else self.v.cpu()}

    def load_state_dict(self, sd):
        if sd["world"] != self.world:
            raise ValueError("ZeRO optimizer state was saved with a different world size")
        self.step_count = sd["step"]
        self.m.copy_(sd["m"])
        if self.v is not None and sd["v"] is not None:
            self.v.copy_(sd["v"])


# ================================================================================================
# ZeRO for the native ResNet program: per-segment reduce-scatter, sharded update, bf16 all-gather
# ================================================================================================
def _reduce_scatter_sum(out: torch.Tensor, inp: torch.Tensor, rank: int, pg) -> None:
    """out = (sum over ranks of inp)[rank part]; gloo has no reduce-scatter: all-reduce + slice."""
    host_sync_for_gloo(inp, pg)
    if dist.get_backend(pg) == "gloo":
        dist.all_reduce(inp, group=pg)
        out.copy_(inp[rank * out.numel():(rank + 1) * out.numel()])
    else:
        dist.reduce_scatter_tensor(out, inp, group=pg)


class SegmentedZero:
    """ZeRO-1/2 over a ResNetProgram's flat buffers (see the module docstring).

    ``seg_ranges``: the [lo, hi) gradient range of every backward segment; each must start on a
    multiple of ``align = 16 * world`` (``ResNetProgram(param_align=...)`` pads the flat layout
    so) and is extended to the next such multiple. ``bn_ranges``: [lo, hi) blocks of fp32
    parameters that must stay exact (the BatchNorm affines)."""

    def __init__(self, prog, optim, seg_ranges, bn_ranges, stage: int = 1, process_group=None, comm=None,
                 collectives: Optional[bool] = None):
        """``comm``: a :class:`~.comm.NativeComm` -- the collectives are then enqueued on the caller's
        stream through the framework's RCCL communicator (capturable into the step's one graph)
        instead of c10d. ``collectives``: take the reduce-scatter / all-gather path even at world 1
        (default: when a process group exists and the engine's ``segmented_graphs`` is on -- the one-GPU RCCL
        rehearsal, where every collective is an identity but runs through RCCL)."""
        if optim.name not in ("sgd", "adam", "adamw"):
            raise ValueError(f"sharded optimizer supports sgd / adam / adamw, not {optim.name!r}")
        K.reject_dampening(optim)
        reject_param_groups(optim, "the sharded (ZeRO) optimizer")
        if stage == 3:
            warnings.warn("native program: ZeRO stage 3 runs as stage 2 (the captured graph needs resident "
                          "parameters; parameter sharding is parallel.fsdp.ShardedDataParallel)")
            stage = 2
        self.stage = stage
        self.prog, self.o, self.pg = prog, optim, process_group
        self.world = dist.get_world_size(process_group) if dist.is_available() and dist.is_initialized() else 1
        self.rank = dist.get_rank(process_group) if self.world > 1 else 0
        self.comm = comm
        if collectives is None:
            collectives = self.world > 1 or (dist.is_available() and dist.is_initialized()
                                             and prog.cfg.segmented_graphs)
        self.coll = bool(collectives)  # the sharded exchange path (reduce-scatter / all-gather) is taken
        W, r = self.world, self.rank
        align = 16 * W
        dev = prog.master.device
        self.parts = []  # (lo, hi, per, own_lo, shard_off)
        off = 0
        for rg in seg_ranges:
            if rg is None:
                continue
            lo, hi = rg
            hi = (hi + align - 1) // align * align
            if lo % align or hi > prog.master.numel():
                raise ValueError(f"segment range {rg} not aligned to {align} (build the program with param_align)")
            per = (hi - lo) // W
            self.parts.append((lo, hi, per, lo + r * per, off))
            off += per
        self.parts.sort()
        for a, b in zip(self.parts, self.parts[1:]):
            if a[1] > b[0]:
                raise ValueError("overlapping segment ranges")
        self.shard_n = off
        self.m = torch.zeros(off, device=dev)
        self.v = torch.zeros(off, device=dev) if optim.name in ("adam", "adamw") else None
        self.gsh = torch.zeros(off, device=dev) if self.coll else None          # reduce-scatter output
        self.p16sh = torch.zeros(off, device=dev, dtype=torch.bfloat16) if self.coll else None  # all-gather input
        self.param16 = prog.param16
        self.work = torch.zeros(4, device=dev)  # [0:2] fp64 sum of squares, [2] clip factor, [3] norm
        self.step_count = 0
        # extra divisor of the reduced gradient next to the world size (the native trainer's gradient
        # accumulation: the gradient is then a sum over world x grad_div micro-batches)
        self.grad_div = 1
        # exact fp32 exchange of the BN affine blocks: this rank's pieces summed with zeros elsewhere
        self.bn_ranges = [tuple(b) for b in bn_ranges]
        nbn = sum(hi - lo for lo, hi in self.bn_ranges)
        self.bnbuf = torch.zeros(max(1, nbn), device=dev) if self.coll else None
        self._bn_own = []  # (buf_off, master_lo, length) of the owned pieces
        bo = 0
        for lo, hi in self.bn_ranges:
            for (_, _, per, own, _) in self.parts:
                a, b = max(lo, own), min(hi, own + per)
                if a < b:
                    self._bn_own.append((bo + a - lo, a, b - a))
            bo += hi - lo
        self.nbn = nbn
        self.bytes_per_step = self.planned_bytes(W)

    def planned_bytes(self, world: int) -> int:
        """Bytes one rank sends per step at ``world`` ranks on a ring: the fp32 reduce-scatter and the
        bf16 all-gather of every segment, plus the fp32 all-reduce of the BN affine blocks (0 at world 1).
        The bench label reports it for the configured world AND for 8 ranks, so a world-1 run still
        states what the exchange will cost."""
        if world <= 1:
            return 0
        n = sum(hi - lo for (lo, hi, *_) in self.parts)
        f = (world - 1) / world
        return int(n * f * (4 + 2) + 2 * f * 4 * self.nbn)

    # ---- helpers ------------------------------------------------------------------------
    def _gpart(self, part):
        lo, hi, per, own, so = part
        return self.prog.grad[own:own + per] if not self.coll else self.gsh[so:so + per]

    # the three collectives: the framework communicator (current stream, capturable) or c10d
    def _rs(self, out, inp):
        if self.comm is not None:
            self.comm.reduce_scatter(out, inp)
        else:
            _reduce_scatter_sum(out, inp, self.rank, self.pg)

    def _ag(self, out, inp):
        if self.comm is not None:
            self.comm.all_gather(out, inp)
        else:
            host_sync_for_gloo(inp, self.pg)
            dist.all_gather_into_tensor(out, inp, group=self.pg)

    def _ar(self, t):
        if self.comm is not None:
            self.comm.all_reduce(t)
        else:
            host_sync_for_gloo(t, self.pg)
            dist.all_reduce(t, group=self.pg)

    def refresh_param16(self) -> None:
        """bf16 copy of the FULL fp32 master (every rank holds it: after the constructor broadcast
        or a checkpoint load)."""
        from ..ops import kernels as K
        K.cast_f32_bf16(self.prog.master, self.param16)

    # ---- collectives (issued between graph replays, on the comm stream) -------------------
    def reduce_range(self, lo: int, hi: int, pre=None) -> None:
        """Reduce-scatter every part inside the backward range [lo, hi). ``pre(plo, phi)``: issued
        right in front of each part's collective on the same stream (the trainer folds its gradient
        accumulator into the part there)."""
        if not self.coll:
            return
        for part in self.parts:
            plo, phi, per, own, so = part
            if lo <= plo < hi:
                if pre is not None:
                    pre(plo, phi)
                self._rs(self.gsh[so:so + per], self.prog.grad[plo:phi])

    def allreduce_norm(self) -> None:
        if self.coll:
            self._ar(self.work[0:2].view(torch.float64))

    def gather(self) -> None:
        """bf16 all-gather of the updated shards into param16; exact fp32 exchange of the BN blocks."""
        if not self.coll:
            return
        for (lo, hi, per, own, so) in self.parts:
            self._ag(self.param16[lo:hi], self.p16sh[so:so + per])
        if self.bn_ranges:  # every rank joins, owner of a BN piece or not
            self.bnbuf.zero_()
            for bo, ml, n in self._bn_own:
                self.bnbuf[bo:bo + n].copy_(self.prog.master[ml:ml + n])
            self._ar(self.bnbuf)
            bo = 0
            for lo, hi in self.bn_ranges:
                self.prog.master[lo:hi].copy_(self.bnbuf[bo:bo + hi - lo])
                bo += hi - lo

    @torch.no_grad()
    def gather_master(self) -> None:
        """Full fp32 master on every rank (collective; before checkpoints / state_dict)."""
        if not self.coll:
            return
        m = self.prog.master
        for (lo, hi, per, own, so) in self.parts:
            buf = torch.empty(hi - lo, device=m.device)
            self._ag(buf, m[own:own + per].contiguous())
            m[lo:hi].copy_(buf)

    # ---- graph-capturable compute -------------------------------------------------------------
    def norm_phase(self) -> None:
        """Local sum of squares of this rank's gradient shard (global-norm clipping)."""
        from ..ops import kernels as K
        self.work.zero_()
        for part in self.parts:
            K.sumsq_accum(self._gpart(part), self.work)

    def update(self, hyper=None, lr=None) -> None:
        """Shard update (fused kernels), writing the bf16 shard for the all-gather (world 1: the
        full bf16 copy directly). Clipping: ``norm_phase`` (+ ``allreduce_norm``) ran before."""
        from ..ops import kernels as K
        o, W = self.o, self.world * self.grad_div
        gs = 1.0 / W
        gsp = None
        if getattr(o, "grad_clip", 0.0):
            gsp = K.clip_factor(self.work, o.grad_clip * W)  # gradients are sums over ranks
        lr = o.lr if lr is None else lr
        for part in self.parts:
            lo, hi, per, own, so = part
            p = self.prog.master[own:own + per]
            g = self._gpart(part)
            p16 = self.param16[own:own + per] if not self.coll else self.p16sh[so:so + per]
            v = None if self.v is None else self.v[so:so + per]
            K.optim_step(o, p, g, self.m[so:so + per], v, p16, step=max(1, self.step_count), lr=lr, grad_scale_ptr=gsp,
                         grad_scale=gs, hyper=hyper)

    def state_dict(self):
        return {"stage": self.stage, "step": self.step_count, "rank": self.rank, "world": self.world,
                "layout": [p[:3] for p in self.parts],
                "m": self.m.cpu(), "v": None if self.v is None else self.v.cpu()}

    def load_state_dict(self, sd):
        if sd["world"] != self.world or [tuple(x) for x in sd.get("layout", [])] != [p[:3] for p in self.parts]:
            raise ValueError("ZeRO optimizer state was saved with a different world size / shard layout")
        self.step_count = sd["step"]
        self.m.copy_(sd["m"])
        if self.v is not None and sd["v"] is not None:
            self.v.copy_(sd["v"])
