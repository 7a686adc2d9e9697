"""Native training step: ResNetProgram + fused optimizer + flat-bucket DDP, replayed as HIP graphs.

One ``NativeTrainer.step()`` = input normalisation (uint8 -> bf16 NHWC4), forward, softmax-CE,
backward, gradient all-reduce (world > 1) and the optimizer update (SGD-momentum / Adam /
AdamW / LARS / LAMB over the flat fp32 master, then the bf16 weight copies are re-derived next step).

Graphs. With world_size == 1 the whole step is ONE captured graph. With world_size > 1 the
step is captured as segments cut where gradient buckets become final (head+layer4 | layer3 |
layer2 | layer1+stem | optimizer); between segment replays the trainer issues the bucket's
RCCL all-reduce on a dedicated comm stream, so the all-reduce of layer4's 15M-parameter bucket
runs under layer3..1's backward (the reference's DDP overlap, SURVEY.md §2.5 M3, without
capturing collectives inside a graph). The optimizer segment waits on the comm stream.

Bucket sizing for xGMI: each segment range is split into chunks of ``bucket_cap_mb`` (default
64 MiB: 8 GPUs x 7 point-to-point links want few, large messages; the 25 MiB NVSwitch-era
default of torch DDP only adds launch latency here).

Validation. ``eval_begin() / eval_step() / eval_end()``: weights and BN coefficients are prepared once
per pass, each batch is one replay of a captured eval forward ending in the metrics kernel
(``K.ce_eval``: loss, top-1, top-k on the device), and the pass ends with its one host read.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Tuple

import numpy as np
import torch
import torch.distributed as dist
import torch.nn as nn

from ..config import (distinct_param_groups, drop_path_probs, has_param_groups, resolve_param_groups,
                      validate_drop_path, validate_loss)
from ..engine_config import EngineConfig
from ..ops import kernels as K
from ..parallel.dist import host_sync_for_gloo
from ..utils import debug as _debug
from ..utils.profiling import PhaseTimer
from .hyper import DeviceHyper
from .mix import MixDraw, MixSampler, auto_augment_stages, validate_auto_augment, validate_mix
from .program import ResNetProgram, release_dead_graphs


@dataclass
class OptimConfig:
    name: str = "sgd"            # sgd | adam | adamw | lars | lamb
    lr: float = 0.1
    momentum: float = 0.9
    dampening: float = 0.0
    nesterov: bool = False
    weight_decay: float = 5e-5
    betas: Tuple[float, float] = (0.9, 0.999)
    eps: float = 1e-8
    grad_clip: float = 0.0       # global-norm clip (DeepSpeed "gradient_clipping")
    trust_coefficient: float = 0.001  # LARS eta (name="lars")
    adapt_1d: bool = False       # LAMB: also decay and adapt BN affine parameters and biases (FusedLamb / apex)
    trust_min: float = 0.0       # LAMB trust-ratio clamp where adapted (0 = unbounded)
    trust_max: float = 0.0
    # parameter groups (sgd | adam | adamw at zero_stage 0; config.resolve_param_groups)
    groups: list = field(default_factory=list)  # [{match, weight_decay?, lr_mult?}, ...]: first match wins
    norm_weight_decay: float = -1.0  # < 0: weight_decay. Every parameter of a normalisation layer
    bias_weight_decay: float = -1.0  # < 0: weight_decay. Biases of all other layers (fc.bias)


@dataclass
class EvalResult:
    """Sums of one evaluation pass (NativeTrainer.eval_end): divide by ``count`` for the means."""
    loss_sum: float
    top1: float   # rows whose label ranks first (ties: the lowest index wins, as in the training step)
    topk: float   # rows whose label is among the k largest logits
    count: int    # rows counted (labels outside [0, classes) are not)
    k: int


class NativeTrainer:
    def __init__(self, model: nn.Module, batch: int, image_hw: Tuple[int, int], device: torch.device,
                 optim: Optional[OptimConfig] = None, label_smoothing: float = 0.0, use_graphs: bool = True,
                 bucket_cap_mb: float = 64.0, allreduce_dtype: torch.dtype = torch.float32,
                 process_group=None, src_hw: Optional[Tuple[int, int]] = None, mean=None, std=None,
                 zero_stage: int = 0, cutmix_alpha: float = 0.0, seed: int = 0,
                 engine: Optional[EngineConfig] = None, grad_accum: int = 1, ema_decay: float = 0.0,
                 ema_warmup: bool = False, mixup_alpha: float = 0.0, mix_prob: float = 1.0,
                 mix_switch_prob: float = 0.5, erase_prob: float = 0.0, erase_mode: str = "const",
                 erase_scale: Tuple[float, float] = (0.02, 1 / 3), erase_ratio: Tuple[float, float] = (0.3, 3.3),
                 auto_augment: Optional[str] = None, ta_num_bins: int = 31, loss: str = "ce",
                 bce_target_threshold: Optional[float] = None, bce_sum_classes: bool = False,
                 ra_num_ops: int = 2, ra_magnitude: int = 9, drop_path_rate: float = 0.0,
                 src_ragged: Optional[Tuple[int, int]] = None):
        validate_loss(loss, bce_target_threshold, bce_sum_classes)
        self.drop_path_rate = validate_drop_path(drop_path_rate)
        validate_mix(mixup_alpha, cutmix_alpha, mix_prob, mix_switch_prob, erase_prob, erase_mode, erase_scale,
                     erase_ratio)
        validate_auto_augment(auto_augment, ta_num_bins, ra_num_ops, ra_magnitude)
        if auto_augment is not None and model.conv1.in_channels != 3:
            raise ValueError(f"auto_augment={auto_augment!r} needs 3-channel images, the model takes "
                             f"{model.conv1.in_channels}")
        self.dev = device
        self.cfg = cfg = engine if engine is not None else EngineConfig.current()
        optim = optim or OptimConfig()
        K.reject_dampening(optim)
        self.pg = process_group
        self.world = dist.get_world_size(process_group) if (dist.is_available() and dist.is_initialized()) else 1
        if zero_stage and optim.name == "lars":
            raise ValueError("LARS runs on the full flat buffer; use zero_stage=0")
        if zero_stage and optim.name == "lamb":
            raise ValueError("LAMB needs every tensor's norms on the full flat buffer; use zero_stage=0")
        if has_param_groups(optim):
            if optim.name in ("lars", "lamb"):
                raise ValueError(f"{optim.name.upper()} has its own per-tensor decay / adapt rule; parameter groups "
                                 f"(groups / norm_weight_decay / bias_weight_decay) work with sgd, adam and adamw")
            if zero_stage:
                raise ValueError("parameter groups need the contiguous flat master; use zero_stage=0 (the sharded "
                                 "layout is not contiguous in flat coordinates)")
        self.ema_decay = float(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        if not 0.0 <= self.ema_decay < 1.0:
            raise ValueError(f"ema_decay must be in [0, 1), got {ema_decay}")
        if zero_stage and self.ema_decay > 0:
            raise ValueError("the weight EMA is not sharded; use zero_stage=0 with ema_decay > 0")
        # ZeRO: segment groups aligned to 16 x world elements (equal per-rank parts) and a flat bf16
        # parameter copy (the all-gather target the weight preparation reads)
        self.prog = ResNetProgram(model, batch, image_hw, device, src_hw=src_hw, mean=mean, std=std,
                                  param_align=16 * self.world if zero_stage else 16, param16=bool(zero_stage),
                                  engine=cfg, src_ragged=src_ragged)
        self.prog.build_backward()
        self.opt = optim
        self.smoothing = label_smoothing
        # the training loss: softmax CE, or binary CE on the same mixed / smoothed targets (K.bce_logits); the
        # program's forward launches one or the other, nothing else in the step sees the choice
        self.loss, self.bce_target_threshold, self.bce_sum_classes = loss, bce_target_threshold, bool(bce_sum_classes)
        self.prog.loss_kind = loss
        self.prog.bce_target_threshold, self.prog.bce_sum_classes = bce_target_threshold, bool(bce_sum_classes)
        # CutMix (Composer's CutMix(alpha), `03_composer/01_cifar_composer_resnet.ipynb:430`): per step a
        # batch permutation and one box are sampled here (host, tiny) and applied on the device by the
        # augment kernel (paste) and the CE kernel (mixed soft targets) inside the captured step
        # MixUp blends the batch with its permutation instead (weight lam ~ Beta(a, a), the CE's lam too);
        # with both alphas set, each step takes one of the two. Random erasing replaces one rectangle per
        # chosen sample before any mixing. Sampling: engine/mix.py; the kernel: K.augment_u8.
        # auto_augment="ta_wide" (TrivialAugmentWide): one of fourteen uint8-space operations per sample, drawn
        # per step into a table that rides in the same arena; the input then runs K.trivial_augment_u8.
        # "ra" (RandAugment) / "aa_imagenet" (AutoAugment's ImageNet policy): K operations in sequence per sample,
        # a stage-major table [K, N, 8] in the same arena region; the input runs K.chain_augment_u8.
        self.cutmix_alpha = float(cutmix_alpha)
        self.mixup_alpha, self.erase_prob, self.erase_mode = float(mixup_alpha), float(erase_prob), erase_mode
        rng_seed = seed + 7919 * (dist.get_rank(process_group) if self.world > 1 else 0)
        self._rng = __import__("numpy").random.default_rng(rng_seed)
        self.last_mix: Optional[MixDraw] = None  # what the last step used
        self._mix, self._mix_ring, self._mix_slot = None, None, 0
        self.auto_augment = auto_augment
        if self.cutmix_alpha > 0 or self.mixup_alpha > 0 or self.erase_prob > 0 or auto_augment is not None:
            self.prog.enable_mix(blend=self.mixup_alpha > 0, erase=self.erase_prob > 0, erase_mode=erase_mode,
                                 seed=rng_seed, ta=auto_augment_stages(auto_augment, ra_num_ops))
            self._mix = MixSampler(self._rng, self.prog.N, self.prog.H, self.prog.W, mixup_alpha=mixup_alpha,
                                   cutmix_alpha=cutmix_alpha, mix_prob=mix_prob, mix_switch_prob=mix_switch_prob,
                                   erase_prob=erase_prob, erase_scale=erase_scale, erase_ratio=erase_ratio,
                                   auto_augment=auto_augment, ta_num_bins=ta_num_bins, ra_num_ops=ra_num_ops,
                                   ra_magnitude=ra_magnitude)
        # stochastic depth, per batch (ResNetProgram.enable_drop_path): every step() call -- micro-steps too --
        # draws u ~ U[0, 1) per gated block from a generator of its own (the mix sampler's sequences do not move),
        # seeded like it by seed and rank: ranks drop different blocks, which is correct because a rank's gates
        # scale its gradients before the collective sums them. The gates reach the device through a pinned ring.
        self.drop_path_p = drop_path_probs(self.drop_path_rate, len(self.prog.blocks))
        self.last_drop_path: Optional[dict] = None  # what the last step used: p, gates, dropped (gated blocks)
        self._drop_rng = self._drop_dev = None
        if self.drop_path_rate > 0:
            self.prog.enable_drop_path(self.drop_path_p)
        if self.prog.drop_gates is not None:
            self._drop_rng = np.random.default_rng([rng_seed, 0x6470])  # ("dp": a stream apart from the mixing's)
            self._drop_p = np.array([self.drop_path_p[l] for l in self.prog.drop_blocks], dtype=np.float64)
            self._drop_keep = (1.0 / (1.0 - self._drop_p)).astype(np.float32)
            self._drop_dev = DeviceHyper(self.prog.drop_gates)
        n = self.prog.n_params
        self.mom = torch.zeros(n, device=device)
        self.mom2 = torch.zeros(n, device=device) if optim.name in ("adam", "adamw", "lamb") else None
        self.hyper = torch.zeros(4, device=device)      # lr, bc1, bc2, window-start flag (device-side, graph-safe)
        self._hyper_dev = DeviceHyper(self.hyper)
        self.clip_work = torch.zeros(4, device=device)
        self.step_count = 0
        # gradient accumulation: k - 1 micro-steps (forward + backward, no collective, no update) add
        # the flat gradient into ``acc``; the k-th call is the boundary step -- the usual step with
        # ``acc`` folded into the gradient before anything consumes it. hyper[3] tells the (captured)
        # accumulate kernel whether a micro-step opens a window (overwrite) or continues one (add).
        self.k = int(grad_accum)
        if self.k < 1:
            raise ValueError("grad_accum must be >= 1")
        self.micro = 0  # position inside the window: calls to step() since the last boundary
        self.acc = torch.zeros(n, device=device) if self.k > 1 else None
        self.micro_graphs: List[Optional[torch.cuda.CUDAGraph]] = []
        # debug mode synchronizes after every kernel, which graph capture forbids; per-phase
        # profiling (DBX_PROFILE=phases: hipEvent timers + roctx ranges) needs eager phases too
        self.phase_timer = PhaseTimer() if "phases" in os.environ.get("DBX_PROFILE", "").split(",") else None
        self.use_graphs = (use_graphs and device.type == "cuda" and not _debug.enabled()
                           and self.phase_timer is None)
        self.graphs: List[Optional[torch.cuda.CUDAGraph]] = []
        self.bucket_cap = int(bucket_cap_mb * (1 << 20) // 4)
        self.ar_dtype = allreduce_dtype
        # segmented = per-segment graphs + side-stream bucket all-reduces. Always on for world > 1;
        # segmented_graphs forces it at world 1 (with an initialised process group) so the
        # RCCL + capture interplay can be rehearsed on a one-GPU box.
        self.segmented = self.world > 1 or (cfg.segmented_graphs and dist.is_available() and dist.is_initialized())
        self.comm_stream = (torch.cuda.Stream(device=device, priority=-1)
                            if self.segmented and device.type == "cuda" else None)
        # comm "native": the DP bucket all-reduces go through the framework's own RCCL communicator
        # (parallel/comm.py) on the comm stream, and the whole step -- backward segments, forked
        # all-reduces, join, optimizer -- is captured as ONE graph instead of per-segment graphs
        # with eager c10d collectives between replays (ZeRO's reduce-scatter / all-gather included)
        # (RCCL process groups, or a one-rank group: under gloo several ranks share one GPU in the
        # one-box tests, and an RCCL communicator would refuse the duplicate device)
        self.ncomm = None
        if self.segmented and device.type == "cuda" and (self.world == 1 or dist.get_backend(process_group) == "nccl"):
            from ..parallel.comm import native_comm_requested, open_verified_comm
            if native_comm_requested(cfg):
                self.ncomm = open_verified_comm(process_group, device)
        # comm_loopback W (test aid, world 1, DP): the framework communicator's all-reduce scales
        # by W in place -- the sum of W identical replicas -- and the update divides by W, so an
        # ordering bug of the one-graph step (a bucket all-reduced before its gradients are final:
        # invisible at world 1, where the collective is the identity) changes the result
        self.loopback = 1
        self.grad_collectives = "c10d"
        if self.ncomm is not None:
            self.grad_collectives = "framework RCCL communicator"
            from ..parallel.collective_plan import direct_enabled
            # the direct two-shot xGMI path for the ranges the plan prices below the ring (opt-in,
            # direct_ar: unmeasured at world >= 2 until a multi-GPU node runs it)
            lb = cfg.comm_loopback
            if lb > 1 and self.world == 1 and zero_stage == 0:
                self.loopback = self.ncomm.loopback = lb
            if direct_enabled(cfg) and zero_stage == 0 and self.world > 1 and self.ncomm.enable_direct(self.prog.grad):
                self.grad_collectives += " + direct xGMI two-shot (small ranges)"
        # Weight gradients next to the per-segment collectives. In the ONE-graph step (framework
        # communicator) the batched side stream (one fork per backward segment, joined one segment
        # later: overlap_wgrad 2) stays on with LATE posts: segment k's
        # gradient range is final only after segment k+1 joins it, so its all-reduce / reduce-scatter
        # is issued after phase k+1 (the last phase posts the last two ranges). Per-segment graphs
        # (c10d collectives between replays) cannot carry a fork across a graph boundary (a capture
        # must end joined), so there -- and with seg_side off -- the round-3 layout stays: weight
        # gradients in order on the main stream, every range posted right after its own phase
        # (per-gradient forks next to the comm stream cost more than they overlapped:
        # profiles/r2s2_multirank/).
        # The per-block layout (the single-GPU default: one side fork per residual block, lazy joins)
        # keeps its schedule in the one-graph step (multirank_layout "block"): every weight gradient of
        # segment k is queued on the side stream by the end of phase k, so the segment's collective is
        # posted on that same stream right behind its last block batch -- in order, no late post -- and
        # only the ranges whose last gradients run on the main stream in a later phase (layer1's
        # block_tail_main gradients, computed after the stem backward) move to the last phase's post.
        self.block_posts = bool(self.segmented and getattr(self.prog, "side_block_default", False)
                                and cfg.multirank_layout == "block" and self.ncomm is not None
                                and cfg.comm_side and device.type == "cuda")
        if self.segmented and getattr(self.prog, "side_block_default", False) and not self.block_posts:
            # the batched side stream with late posts (round 5's multi-rank layout; the c10d
            # per-segment graphs can carry no fork across a graph boundary)
            p, pol = self.prog, cfg.policy
            p.side_block, p.side_batch = False, True
            p.side_defer = cfg.side_defer if cfg.side_defer is not None else pol.small(p.fwd_flops)
            p.lazy_join = cfg.lazy_join if cfg.lazy_join is not None else pol.tiny(p.fwd_flops)
            p.stem_wg_main = cfg.stem_wg_main if cfg.stem_wg_main is not None else pol.small(p.fwd_flops)
            # (with its collectives on the side stream the batched layout keeps the 64-CU reservation:
            # world-1 RCCL one-graph step with a real collective kernel, headline +0.5-1.1 % over 128,
            # TinyImageNet +0.1 %, profiles/r5_cu_reserve/sweep_late.txt)
            if cfg.side_cu_reserve is None:
                p.side_cu_reserve = 0 if pol.tiny(p.fwd_flops) else 64
        seg_side = cfg.seg_side and (self.ncomm is not None or not self.use_graphs)
        if self.segmented and cfg.overlap_wgrad is None and not seg_side:
            self.prog.overlap_wgrad = False
        self.late_posts = bool(self.segmented and device.type == "cuda" and seg_side and self.prog.overlap_wgrad
                               and self.prog.side_batch)
        if self.segmented and not self.late_posts:
            # per-segment collectives right after their own phase need each segment's weight gradients
            # final at its end: no batched side stream (it joins a segment late)
            self.prog.side_batch = False
        if self.segmented and not cfg.comm_side:
            self.prog.lazy_join = False  # (a separate comm stream orders after the main stream's joins)
        # comm_side (default on): in the one-graph step the collectives run on the weight-gradient
        # side stream itself (behind the batch that finished their range) instead of a third stream.
        # Under DEBUG_HIP_FORCE_GRAPH_QUEUES=2 a separate comm branch took the graph's second hardware
        # queue and pushed the weight-gradient branch onto the main chain's queue: with a real
        # collective in the graph (world-1 comm_loopback=2) TinyImageNet fell from 97.9k to 85.5k
        # img/s and the headline by 1.2 % (profiles/r5_comm_queue/). The joins then wait on an event
        # behind each batch, not on the collectives queued after it.
        self.comm_side = bool(self.ncomm is not None and (self.late_posts or self.block_posts)
                              and device.type == "cuda" and cfg.comm_side)
        if self.comm_side:
            self.comm_stream = self.prog.side_stream()
            self.prog.event_joins = True
            if cfg.side_defer is None:
                self.prog.side_defer = True  # (the side branch then keeps its own hardware queue)
        if self.segmented and ((self.prog.side_block and not self.block_posts) or not self.comm_side):
            # collectives posted per segment need that segment's weight gradients joined at its end
            # (lazy joins only where the collectives ride the side stream behind the batches)
            self.prog.lazy_join = False
        self.flip = None
        self.seg_ranges = self._segment_ranges()
        self.zero = None
        if zero_stage:
            from ..parallel.zero import SegmentedZero
            self.zero = SegmentedZero(self.prog, optim, self.seg_ranges, self.prog.bn_param_blocks(),
                                      stage=zero_stage, process_group=process_group, comm=self.ncomm,
                                      collectives=self.segmented)
            self.zero.grad_div = self.k
            self.mom = self.zero.m  # shard-sized optimizer state only
            self.mom2 = self.zero.v
        self.group_runs, self._group_values = self._param_group_runs()
        self.lars = self._lars_segments() if optim.name == "lars" else None
        self.lamb = self._lars_segments(adapt_all=optim.adapt_1d) if optim.name == "lamb" else None
        # weight EMA (ema_decay > 0): ``ema`` shadows the flat master and is moved by the optimizer
        # kernels themselves (fused variant); ``ema_bn`` shadows every BN's running_mean / running_var
        # (module buffers outside the master: one table-driven launch in the optimizer phase). 1 - d_t
        # reaches the captured step through a device scalar of its own (hyper's layout is untouched).
        self.ema = self.ema_bn = None
        if self.ema_decay > 0:
            self._alloc_ema()
        # evaluation pass (eval_begin / eval_step / eval_end): its own fp64 [loss sum, top-1, top-k, count]
        # and the batch's valid-row count as a device scalar, so one captured graph serves short batches
        self.eval_stats = torch.zeros(4, device=device, dtype=torch.float64)
        self.eval_nvalid = torch.zeros(1, device=device, dtype=torch.int32)
        self.eval_graph: Optional[torch.cuda.CUDAGraph] = None
        self._eval_on = False
        self._eval_k = self._eval_graph_k = 0
        self._eval_warm = 0
        self._eval_n: Optional[int] = None  # what eval_nvalid holds
        self._build_phases()
        self.opt_ranges = self._optimizer_ranges()
        # broadcast initial parameters from rank 0 (DDP constructor semantics, M2)
        if self.world > 1:
            src = 0 if process_group is None else dist.get_global_rank(process_group, 0)
            host_sync_for_gloo(self.prog.master, process_group)
            dist.broadcast(self.prog.master, src, group=process_group)
            for bn in self.prog.bns:
                dist.broadcast(bn.mod.running_mean, src, group=process_group)
                dist.broadcast(bn.mod.running_var, src, group=process_group)
        if self.zero is not None:
            self.zero.refresh_param16()
        if self.ema is not None:
            self._seed_ema()

    # ----------------------------------------------------------------------------------
    def _alloc_ema(self):
        p, dev = self.prog, self.dev
        self.ema = torch.zeros(p.n_params, device=dev)
        # one flat buffer, [mean, var] per BN in prog.bns order, each at a 16-byte aligned offset
        offs, o = [], 0
        for bn in p.bns:
            offs.append(o)
            o += 2 * ((bn.C + 3) // 4 * 4)
        self.ema_bn = torch.zeros(o, device=dev)
        self.ema_bn_views = []
        pairs = []
        for bn, o in zip(p.bns, offs):
            c = (bn.C + 3) // 4 * 4
            mean, var = self.ema_bn[o:o + bn.C], self.ema_bn[o + c:o + c + bn.C]
            self.ema_bn_views.append((mean, var))
            pairs += [(mean, bn.mod.running_mean), (var, bn.mod.running_var)]
            # what an evaluation from the average hands bn_eval_coeff (program._bn_fwd)
            bn.ema_eval = (self.ema[bn.off_w:bn.off_w + bn.C], self.ema[bn.off_b:bn.off_b + bn.C], mean, var)
        p.bn_eval_table_ema = p.pack_bn_eval(ema=True)  # an evaluation pass from the average (eval_begin)
        self._ema_bn_desc = K.pack_ema_desc(pairs, dev)
        self._ema_bn_n, self._ema_bn_max = len(pairs), max(bn.C for bn in p.bns)
        self.ema_hyper = torch.zeros(1, device=dev)  # 1 - d_t (device-side, graph-safe)
        self._ema_hyper_dev = DeviceHyper(self.ema_hyper)

    def _seed_ema(self):
        """The average starts at (a copy of) the current parameters and running statistics."""
        with torch.no_grad():
            self.ema.copy_(self.prog.master)
            for bn, (mean, var) in zip(self.prog.bns, self.ema_bn_views):
                mean.copy_(bn.mod.running_mean)
                var.copy_(bn.mod.running_var)

    def ema_decay_at(self, t: int) -> float:
        """The decay d_t of optimizer step ``t`` (1-based): ``ema_decay``, or with ``ema_warmup``
        min(ema_decay, (1 + t) / (10 + t)) (the timm / TF rule)."""
        if self.ema_warmup:
            return min(self.ema_decay, (1.0 + t) / (10.0 + t))
        return self.ema_decay

    def _ema_kw(self, lo: int, hi: int) -> dict:
        """The fused-average arguments of an optimizer launch over master[lo:hi] (none when off)."""
        if self.ema is None:
            return {}
        return {"ema": self.ema[lo:hi], "ema_hyper": self.ema_hyper,
                "ema_one_minus_decay": 1.0 - self.ema_decay}

    def _param_group_runs(self):
        """Parameter groups (OptimConfig.groups / norm_weight_decay / bias_weight_decay): every tensor's
        (weight_decay, lr_mult), resolved from its name and kind (a BN's parameters are "norm", any other
        ``.bias`` is "bias": the rule of _lars_segments), and the run table of the flat master the SGD / Adam
        kernels read -- neighbours with equal values merged; the alignment padding between tensors joins
        the run before it (master and gradient are zero there). (None, None) when nothing is set: the
        trainer then runs exactly the plain launches."""
        rs = self.prog.param_ranges
        bn_names = {f"{bn.name}." for bn in self.prog.bns}
        kinds = [(r[0], "norm" if any(r[0].startswith(b) for b in bn_names)
                  else "bias" if r[0].endswith(".bias") else "weight") for r in rs]
        values = resolve_param_groups(kinds, self.opt)
        if values is None:
            return None, None
        runs = []
        for (_, off, _), val in sorted(zip(rs, values), key=lambda t: t[0][1]):
            if not runs:
                runs.append((0,) + val)
            elif val != runs[-1][1:]:
                runs.append((off,) + val)
        return K.pack_opt_runs(runs, self.prog.n_params, self.dev), values

    def param_group_table(self):
        """``[(name, weight_decay, lr_mult)]`` per parameter tensor, in flat-buffer order: what the optimizer
        applies (without groups: the one weight decay and 1.0; LARS / LAMB keep their own rule)."""
        rs = self.prog.param_ranges
        values = self._group_values or [(float(self.opt.weight_decay), 1.0)] * len(rs)
        return [(r[0], wd, lm) for r, (wd, lm) in zip(rs, values)]

    def param_group_summary(self):
        """``[(weight_decay, lr_mult, tensors, elements)]`` per distinct group, for the log."""
        rs, tab = self.prog.param_ranges, self.param_group_table()
        return [(wd, lm, sum(1 for t in tab if t[1:] == (wd, lm)),
                 sum(r[2] for r, t in zip(rs, tab) if t[1:] == (wd, lm)))
                for wd, lm in distinct_param_groups([t[1:] for t in tab])]

    def _wd_kw(self, lo: int) -> dict:
        """The weight-decay arguments of an SGD / Adam launch over master[lo:]: the scalar, or with
        parameter groups the run table (which carries the decays) and the slice's place in it."""
        if self.group_runs is None:
            return {"weight_decay": self.opt.weight_decay}
        return {"weight_decay": 0.0, "runs": self.group_runs, "run_base": lo}

    def _segment_ranges(self):
        """Contiguous [lo, hi) of every backward segment's gradients (None: no parameters)."""
        out = []
        for rs in self.prog.segment_param_ranges():
            if not rs:
                out.append(None)
                continue
            out.append((min(r[1] for r in rs), max(r[1] + (r[2] + 15) // 16 * 16 for r in rs)))
        return out

    def _build_phases(self):
        """Phases = (name, fn, post): ``fn`` is graph-captured (no collectives); ``post`` is what the
        multi-rank path issues on the comm stream after the phase -- a gradient range (all-reduce,
        or ZeRO reduce-scatter) or a callable (ZeRO norm all-reduce / parameter all-gather)."""
        p = self.prog
        segs = p._segments

        def fwd_phase():
            # bf16 weights + BN-statistics zeroing + every BN's num_batches_tracked, one launch
            p.prepare_weights(step=True)
            p.load_input_u8(self.flip)
            p.forward(smoothing=self.smoothing)

        phases: List[Tuple[str, Callable, Optional[Tuple[int, int]]]] = []
        # phase 0 = forward + first backward segment
        first_name, first_fn = segs[0]
        phases.append(("fwd+" + first_name, lambda: (fwd_phase(), first_fn()), self.seg_ranges[0]))
        for (name, fn), rg in zip(segs[1:], self.seg_ranges[1:]):
            phases.append((name, fn, rg))
        if self.segmented and self.late_posts:
            # batched side stream: phase k completes segment k-1's weight gradients (see __init__)
            rgs = [ph[2] for ph in phases]
            shifted = [None] + rgs[:-1]
            shifted[-1] = [r for r in (rgs[-2], rgs[-1]) if r is not None] if len(rgs) > 1 else rgs[-1]
            phases = [(n, fn, post) for (n, fn, _), post in zip(phases, shifted)]
        elif self.segmented and self.block_posts:
            # per-block layout: each range at its own phase's end, layer1's with the stem's when its last
            # block's tail gradients run on the main stream after the stem backward (see __init__)
            if self.prog.block_tail_main > 0 and len(phases) > 1:
                rgs = [ph[2] for ph in phases]
                shifted = rgs[:-2] + [None, [r for r in (rgs[-2], rgs[-1]) if r is not None]]
                phases = [(n, fn, post) for (n, fn, _), post in zip(phases, shifted)]
        elif self.segmented:
            phases = self._merge_phases(phases)
        z = self.zero
        # ZeRO + clipping with collectives: the shard's sum of squares is all-reduced between phases
        self._zero_norm_separate = z is not None and bool(self.opt.grad_clip) and self.segmented
        if self._zero_norm_separate:
            phases.append(("opt_norm", z.norm_phase, z.allreduce_norm))
        phases.append(("optimizer", self._optimizer_phase, z.gather if z is not None else None))
        self.phases = phases
        # micro-step (grad_accum > 1): the same forward / backward phases without their collectives
        # (DDP's no_sync), the optimizer phases replaced by one pass adding the gradient into ``acc``
        self.micro_phases = None
        if self.k > 1:
            self.micro_phases = [(n, fn, None) for n, fn, _ in phases if n not in ("optimizer", "opt_norm")]
            self.micro_phases.append(("accumulate", self._accumulate_phase, None))

    def _optimizer_ranges(self):
        """The optimizer inside the backward (engine field ``overlap_optimizer``): SGD / Adam are
        element-wise, so each backward segment's parameters are updated as soon as that segment's
        gradients are final (and, at world > 1, all-reduced), on the weight-gradient side stream right
        behind the segment's last block batch (and its collective) -- the step no longer ends with a
        serial update of every parameter. Per phase the ranges to update after it; the last phase's
        (and layer1's, whose last block's tail weight gradients run on the main stream after the stem
        backward) go on the main stream after the final join; element ranges no segment covers are
        updated in the optimizer phase. Off (None) for clipping / LARS / LAMB (global or per-tensor norms), ZeRO (its own
        sharded update), the c10d per-segment graphs and the batched side-stream layouts."""
        p, cfg = self.prog, self.cfg
        if self.k > 1:  # (the accumulator is folded in at the top of the optimizer phase)
            return None
        if not (cfg.overlap_optimizer != 0 and self.zero is None and self.lars is None and self.lamb is None
                and not (self.opt.grad_clip and self.opt.grad_clip > 0)
                and p.side_block and p.overlap_wgrad and (not self.segmented or self.block_posts)):
            return None
        nph = len(self.seg_ranges)
        per = [[r] if r is not None else [] for r in self.seg_ranges]
        if nph > 1 and p.block_tail_main > 0:
            per[-1] = per[-2] + per[-1]
            per[-2] = []
        if cfg.overlap_optimizer > 0:  # only the first N segments inside the backward
            per = [rs if k < cfg.overlap_optimizer else [] for k, rs in enumerate(per)]
        covered = sorted(r for rs in per for r in rs)
        gaps, pos = [], 0  # (merged: the segments are contiguous in backward order, one launch each gap)
        for lo, hi in covered:
            if lo > pos:
                gaps.append((pos, lo))
            pos = max(pos, hi)
        if pos < p.n_params:
            gaps.append((pos, p.n_params))
        if not covered:
            return None
        return {"per_phase": per, "gaps": gaps}

    def _update_range(self, lo: int, hi: int, gsp=None):
        """The SGD / Adam update of master[lo:hi] from the reduced gradient sum (``gsp``: the clip factor)."""
        p = self.prog
        K.optim_step(self.opt, p.master[lo:hi], p.grad[lo:hi], self.mom[lo:hi],
                     None if self.mom2 is None else self.mom2[lo:hi], grad_scale_ptr=gsp,
                     grad_scale=1.0 / (self.world * self.loopback * self.k), hyper=self.hyper,
                     **self._wd_kw(lo), **self._ema_kw(lo, hi))

    def _after_phase_updates(self, i: int):
        """Issue phase i's parameter updates (see _optimizer_ranges)."""
        if self.opt_ranges is None:
            return
        rs = self.opt_ranges["per_phase"][i] if i < len(self.opt_ranges["per_phase"]) else []
        if not rs:
            return
        last = i == len(self.opt_ranges["per_phase"]) - 1
        if self.dev.type != "cuda" or last:
            for r in rs:  # (the last phase ended with the final join: on the main stream)
                self._update_range(*r)
            return
        run = (lambda rs=rs: [self._update_range(*r) for r in rs])
        if not self.prog.defer_on_side(run):  # behind the deferred batch (and collective), or now
            side = self.prog.side_stream()
            side.wait_stream(torch.cuda.current_stream(self.dev))
            with torch.cuda.stream(side):
                run()
            self.prog._side_pending = True  # (the next join, at the latest the final one, waits for it)

    def _merge_phases(self, phases):
        """Optional coarser graph segmentation of the multi-rank path: seg_groups "3:3" merges
        the six backward segments into two graphs (one all-reduce cut after layer3). Default: one
        graph per backward segment. Measured over RCCL on one MI355X (world-1 process group with
        segmented_graphs=1, ResNet-50 b1024, wgrad side stream on): 6 segments 13.98k / 14.03k
        img/s, 2 segments 14.05k / 14.07k, one backward graph 13.99k / 14.00k, plain single graph
        14.45k / 14.43k (profiles/r2s2_multirank/step_layout_ab.txt) -- boundaries are not what
        the segmented path cost: the wgrad side stream next to the comm streams was (now off in
        this mode, see __init__). The finer split (more overlap, smallest exposed tail) stays.
        Groups merge only when their gradient ranges are disjoint and in order."""
        spec = self.cfg.seg_groups
        if not spec:
            return phases
        sizes = [int(x) for x in spec.split(":") if x.strip()]
        sizes = [x for x in sizes if x > 0]
        if sum(sizes) != len(phases):
            raise ValueError(f"seg_groups={spec!r} does not cover {len(phases)} backward segments")
        merged, pos = [], 0
        for sz in sizes:
            grp = phases[pos:pos + sz]
            pos += sz
            rgs = sorted(rg for _, _, rg in grp if rg is not None)
            # consecutive phases own consecutive parameter groups (at most alignment padding between)
            if any(a[1] > b[0] for a, b in zip(rgs, rgs[1:])):
                return phases  # non-adjacent gradient ranges: keep one segment per phase
            fns = [fn for _, fn, _ in grp]
            merged.append(("+".join(nm for nm, _, _ in grp),
                           (lambda fns=fns: [f() for f in fns]),
                           (rgs[0][0], rgs[-1][1]) if rgs else None))
        return merged

    def _lars_segments(self, adapt_all: bool = False):
        """Per-tensor segments of the flat buffer for LARS and LAMB; conv / fc weights are adapted (and
        decayed), BN affine parameters and biases are not (the usual large-batch recipe) unless
        ``adapt_all`` (LAMB's ``adapt_1d``: every tensor, as DeepSpeed's FusedLamb and apex do)."""
        rs = self.prog.param_ranges
        dev = self.dev
        off = torch.tensor([r[1] for r in rs], dtype=torch.int32, device=dev)
        ln = torch.tensor([r[2] for r in rs], dtype=torch.int32, device=dev)
        bn_names = {f"{bn.name}." for bn in self.prog.bns}
        adapt = torch.tensor([int(adapt_all or
                                  (r[0].endswith(".weight") and not any(r[0].startswith(b) for b in bn_names)))
                              for r in rs], dtype=torch.int32, device=dev)
        return off, ln, adapt, torch.zeros(K.LARS_MAX_BLOCKS * 2 * len(rs), device=dev, dtype=torch.float64), max(r[2] for r in rs)

    def _accumulate_phase(self):
        K.grad_accum(self.acc, self.prog.grad, flag=self.hyper[3:4])

    def _fold(self, lo: int, hi: int):
        """Boundary step: grad[lo:hi] += acc[lo:hi] (on the current stream, before the range's consumer)."""
        K.grad_accum(self.prog.grad[lo:hi], self.acc[lo:hi])

    def _optimizer_phase(self):
        p, o = self.prog, self.opt
        if self.k > 1 and not self.segmented:
            # no per-range collective folded the accumulator in: once over the whole buffer
            self._fold(0, p.grad.numel())
        if self.ema is not None:
            # the BN running statistics are final since the forward: all 2 x len(bns) buffers, one launch
            K.ema_update_multi(self._ema_bn_desc, self._ema_bn_n, self._ema_bn_max,
                               one_minus_decay=1.0 - self.ema_decay, hyper=self.ema_hyper)
        if self.zero is not None:
            # ZeRO-1/2: update this rank's shard of the fp32 master with its shard of the optimizer
            # state (the reduce-scatter and the all-gather run around this phase, not inside it:
            # the phase is captured at every world size). lr / bias corrections come from the
            # device-side hyper tensor so a replayed step follows set_lr() and the step count.
            if o.grad_clip and not self._zero_norm_separate:
                self.zero.norm_phase()
            self.zero.update(hyper=self.hyper)
            return
        if self.opt_ranges is not None:  # updated inside the backward: only uncovered ranges remain
            for r in self.opt_ranges["gaps"]:
                self._update_range(*r)
            return
        gsp = None
        gdiv = self.world * self.loopback * self.k  # the reduced gradient is a sum over gdiv micro-batches
        if o.grad_clip and o.grad_clip > 0:
            # clip on the averaged gradient: factor computed on device (no host sync)
            K.global_norm_clip_factor(p.grad, o.grad_clip * gdiv, self.clip_work)
            gsp = self.clip_work[2:3]
        if self.lars is not None:
            # the clip factor scales the gradient before the trust ratios, as torch's
            # clip_grad_norm_ + LARS does on the autograd engine
            if gsp is not None:
                p.grad.mul_(gsp)
            off, ln, adapt, norms, mx = self.lars
            K.lars_scale(p.master, p.grad, off, ln, adapt, norms, grad_scale=1.0 / gdiv,
                         eta=o.trust_coefficient, weight_decay=o.weight_decay, max_len=mx)
            K.optim_step(o, p.master, p.grad, self.mom, None, weight_decay=0.0, grad_scale=1.0, hyper=self.hyper,
                         **self._ema_kw(0, p.n_params))
            return
        gscale = 1.0 / gdiv
        if self.lamb is not None:
            # one call over the whole flat buffer; the clip factor multiplies the gradient scale through
            # the pointer, as on the Adam path (the moments see the clipped gradient)
            off, ln, adapt, norms, mx = self.lamb
            K.lamb_step(p.master, p.grad, self.mom, self.mom2, off, ln, adapt, norms, None, lr=o.lr,
                        beta1=o.betas[0], beta2=o.betas[1], eps=o.eps, weight_decay=o.weight_decay, step=1,
                        trust_min=o.trust_min, trust_max=o.trust_max, grad_scale_ptr=gsp, grad_scale=gscale,
                        hyper=self.hyper, max_len=mx, **self._ema_kw(0, p.n_params))
            return
        self._update_range(0, p.n_params, gsp)

    # ----------------------------------------------------------------------------------
    def _post(self, post):
        if post is None:
            return
        if callable(post):
            post()
        elif isinstance(post, list):  # late posts: several gradient ranges after one phase
            for rg in post:
                self._post(rg)
        elif self.zero is not None:
            self.zero.reduce_range(*post, pre=self._fold if self.k > 1 else None)
        else:
            if self.k > 1:  # the window's sum goes into the collective: fold right in front of it
                self._fold(*post)
            self._allreduce_range(*post)

    def _allreduce_range(self, lo: int, hi: int):
        g = self.prog.grad
        if self.ncomm is not None:  # enqueued on the current (comm) stream; capturable
            from ..parallel.collective_plan import plan_allreduce
            esz = torch.tensor([], dtype=self.ar_dtype).element_size()
            plan = plan_allreduce(hi - lo, esz, self.world, self.bucket_cap,
                                  allow_direct=self.ncomm.direct is not None and self.ar_dtype == torch.float32)
            for a, b in plan.buckets:
                chunk = g[lo + a:lo + b]
                if self.ar_dtype == torch.float32:
                    self.ncomm.all_reduce(chunk)  # direct path when the plan picked it (NativeComm.all_reduce)
                else:
                    buf = chunk.to(self.ar_dtype)
                    self.ncomm.all_reduce(buf)
                    chunk.copy_(buf)
            return
        host_sync_for_gloo(g, self.pg)
        pos = lo
        while pos < hi:
            end = min(hi, pos + self.bucket_cap)
            chunk = g[pos:end]
            if self.ar_dtype == torch.float32:
                dist.all_reduce(chunk, group=self.pg)
            else:
                buf = chunk.to(self.ar_dtype)
                dist.all_reduce(buf, group=self.pg)
                chunk.copy_(buf)
            pos = end

    def _sample_mix(self):
        """This step's mixing (engine/mix.py: none / MixUp / CutMix, erase boxes) from the trainer's
        generator, written to the program's device scalars and tables through pinned buffers. With only
        ``cutmix_alpha`` set: the draws and the three copies the trainer has always made."""
        p = self.prog
        d = self.last_mix = self._mix.sample()
        if p.mix_arena is not None:
            # the mixing kernel's state is one arena (ResNetProgram.enable_mix): one copy per step from a
            # small pinned ring whose slot is rewritten only after its previous copy completed (engine/hyper.py:
            # a pinned allocation per step is enough host work to stall a ~1 ms step)
            N = p.N
            if self._mix_ring is None:
                cuda = self.dev.type == "cuda"
                words = p.mix_arena.numel()  # (5 N + 6, and 8 N more per stage of the auto-augment table)
                self._mix_ring = [(torch.zeros(words, dtype=torch.int32).pin_memory() if cuda
                                   else torch.zeros(words, dtype=torch.int32),
                                   torch.cuda.Event() if cuda else None) for _ in range(4)]
            buf, ev = self._mix_ring[self._mix_slot]
            self._mix_slot = (self._mix_slot + 1) % len(self._mix_ring)
            if ev is not None:
                ev.synchronize()  # (a no-op for a fresh event)
            h = buf.numpy()
            h[:N] = d.perm
            h[N:N + 4] = d.box
            h[N + 4:N + 6].view("float32")[:] = (d.lam, d.blend)
            h[N + 6:5 * N + 6] = d.erase.reshape(-1) if d.erase is not None else 0
            if d.ta is not None:
                h[5 * N + 6:] = d.ta.reshape(-1)
            p.mix_arena.copy_(buf, non_blocking=True)
            if ev is not None:
                ev.record()
            return
        host = [(p.mix_perm, torch.from_numpy(d.perm)),
                (p.mix_box, torch.tensor(d.box, dtype=torch.int32)),
                (p.mix_lam, torch.tensor([d.lam], dtype=torch.float32))]
        if self.dev.type == "cuda":
            host = [(dst, src.pin_memory()) for dst, src in host]
        self._mix_host = host  # keep the pinned sources alive until the copies ran
        for dst, src in host:
            dst.copy_(src, non_blocking=True)

    def _sample_drop_path(self):
        """This step's gates: block l is dropped (gate 0) when u < p_l, else kept with gate fl32(1 / (1 - p_l))."""
        u = self._drop_rng.random(len(self._drop_p))
        dropped = u < self._drop_p
        gates = np.where(dropped, np.float32(0.0), self._drop_keep)
        self.last_drop_path = {"p": self._drop_p.tolist(), "gates": [float(g) for g in gates],
                               "dropped": [l for l, d in zip(self.prog.drop_blocks, dropped) if d]}
        self._drop_dev.set(self.last_drop_path["gates"])

    def drop_path_summary(self) -> dict:
        """The stochastic-depth settings, for logging."""
        gated = self.prog.drop_blocks
        return {"drop_path_rate": self.drop_path_rate, "mode": "batch", "blocks": len(self.prog.blocks),
                "gated_blocks": len(gated), "p_max": max(self.drop_path_p) if gated else 0.0,
                "kernel": "gate_scale_multi" if gated else None,
                "launches_per_step": (1 + len(self.prog._gate_bwd)) if gated else 0}

    def loss_summary(self) -> dict:
        """The training-loss settings, for logging."""
        return {"loss": self.loss, "label_smoothing": self.smoothing,
                "bce_target_threshold": self.bce_target_threshold, "bce_sum_classes": self.bce_sum_classes,
                "kernel": "bce_logits" if self.loss == "bce" else "softmax_ce"}

    def mix_summary(self) -> dict:
        """The batch-mixing settings, for logging."""
        m = self._mix
        return {"mixup_alpha": self.mixup_alpha, "cutmix_alpha": self.cutmix_alpha,
                "mix_prob": m.mix_prob if m else 1.0, "mix_switch_prob": m.mix_switch_prob if m else 0.5,
                "erase_prob": self.erase_prob, "erase_mode": self.erase_mode,
                "erase_scale": m.erase_scale if m else None, "erase_ratio": m.erase_ratio if m else None,
                "auto_augment": self.auto_augment, "ta_num_bins": m.ta_num_bins if m else 31,
                **({"num_ops": self.prog.ta_stages, "magnitude": m.ra_magnitude if self.auto_augment == "ra" else None}
                   if self.auto_augment in ("ra", "aa_imagenet") else {}),
                "kernel": ("chain_augment_u8" if self.prog.ta_stages > 1 else
                           "trivial_augment_u8" if self.prog.ta_ops is not None else
                           "augment_mix_u8" if self.prog.mix_blend is not None else "augment_u8")}

    def _set_hyper(self, boundary: bool = True):
        o = self.opt
        # optimizer steps, not micro-steps, are counted (Adam's bias corrections, zero.step_count); a
        # micro-step carries the values of the update its window ends with
        if boundary:
            self.step_count += 1
        t = self.step_count if boundary else self.step_count + 1
        first = 1.0 if (self.k > 1 and self.micro == 0) else 0.0  # this micro-step opens a window
        if o.name in ("sgd", "lars"):
            vals = [o.lr, 1.0, 1.0, first]
        else:
            vals = [o.lr, 1.0 - o.betas[0] ** t, 1.0 - o.betas[1] ** t, first]
        self._hyper_dev.set(vals)
        if self.ema is not None:
            # 1 - d_t in double; the copy to the fp32 device scalar is its one rounding. (A micro-step
            # launches no EMA kernel; it carries the value of the update its window ends with.)
            self._ema_hyper_dev.set([1.0 - self.ema_decay_at(t)])

    @property
    def grad_accum(self) -> int:
        """Micro-batches per optimizer step."""
        return self.k

    @property
    def at_boundary(self) -> bool:
        """True when the next ``step()`` applies the optimizer update (always, without accumulation)."""
        return self.micro == self.k - 1

    def set_lr(self, lr: float):
        self.opt.lr = float(lr)

    def _waits_comm(self, i: int, name: str) -> bool:
        # the optimizer phases consume the reduced gradients / norm; the first phase of a step
        # consumes the previous step's all-gathered parameters
        # (inside the one-graph capture the comm stream joins only after its first fork: no wait on
        # work recorded outside the capture)
        first = i == 0 and not getattr(self, "_capturing_one", False)
        # (the accumulate phase of a micro-step reads the whole gradient like the optimizer does)
        return self.segmented and (first or name in ("optimizer", "opt_norm", "accumulate"))

    def _run_phases_eager(self, micro: bool = False):
        phases = self.micro_phases if micro else self.phases
        if self.dev.type != "cuda":  # CPU (reference ops; gloo collectives, synchronous)
            for i, (name, fn, post) in enumerate(phases):
                fn()
                if self.segmented and post is not None:
                    self._post(post)
                self._after_phase_updates(i)
            return
        cur = torch.cuda.current_stream(self.dev)
        for i, (name, fn, post) in enumerate(phases):
            if self._waits_comm(i, name):
                self.prog.launch_pending()
                # (a micro-step's one-graph capture forks no comm stream: nothing of it to wait for)
                if not (micro and getattr(self, "_capturing_one", False)):
                    cur.wait_stream(self.comm_stream)
            if self.phase_timer is not None:
                with self.phase_timer.phase(name):
                    fn()
            else:
                fn()
            if post is not None and self.segmented:
                # (comm_side with a deferred side batch: the collective goes in behind the batch,
                # under the batch's fork event -- the main stream's state at this phase's end)
                if not (self.comm_side and self.prog.defer_on_side(lambda post=post: self._post(post))):
                    self.comm_stream.wait_stream(cur)
                    with torch.cuda.stream(self.comm_stream):
                        self._post(post)
            self._after_phase_updates(i)

    def _graph_phases(self, micro: bool = False):
        return self.micro_phases if micro else self.phases

    def _capture(self, micro: bool = False):
        """Capture each phase (or the whole step when not segmented) into HIP graphs: the full /
        boundary step into ``graphs``, the micro-step of gradient accumulation into ``micro_graphs``."""
        release_dead_graphs(self.dev)
        s = torch.cuda.Stream(device=self.dev)
        s.wait_stream(torch.cuda.current_stream(self.dev))
        pool = torch.cuda.graph_pool_handle()
        graphs: List[Optional[torch.cuda.CUDAGraph]] = []
        if micro:
            self.micro_graphs = graphs
        else:
            self.graphs = graphs
        # thread-local capture whenever a process group exists: its watchdog thread polls the
        # completion events of earlier collectives while we capture, and under the default
        # global mode such a query from another thread invalidates the capture
        mode = "thread_local" if (dist.is_available() and dist.is_initialized()) else "global"
        with torch.cuda.stream(s):
            if self.ncomm is not None:
                # one graph: the comm-stream fork / join of every bucket is recorded as graph edges
                g = torch.cuda.CUDAGraph()
                self._capturing_one = True
                try:
                    with torch.cuda.graph(g, pool=pool, stream=s, capture_error_mode=mode):
                        self._run_phases_eager(micro)
                        self.prog.launch_pending()
                        if not micro:
                            torch.cuda.current_stream(self.dev).wait_stream(self.comm_stream)
                finally:
                    self._capturing_one = False
                graphs.append(g)
            elif not self.segmented:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, pool=pool, stream=s, capture_error_mode=mode):
                    for i, (_, fn, _) in enumerate(self._graph_phases(micro)):
                        fn()
                        self._after_phase_updates(i)
                    self.prog.launch_pending()
                graphs.append(g)
            else:
                for _, fn, _ in self._graph_phases(micro):
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, pool=pool, stream=s, capture_error_mode=mode):
                        fn()
                    graphs.append(g)
        torch.cuda.current_stream(self.dev).wait_stream(s)
        torch.cuda.synchronize(self.dev)

    def _replay(self, micro: bool = False):
        cur = torch.cuda.current_stream(self.dev)
        graphs = self.micro_graphs if micro else self.graphs
        if not self.segmented or self.ncomm is not None:
            if self.ncomm is not None:
                cur.wait_stream(self.comm_stream)  # eager warm-up collectives
            graphs[0].replay()
            return
        for i, ((name, _, post), g) in enumerate(zip(self._graph_phases(micro), graphs)):
            if self._waits_comm(i, name):
                cur.wait_stream(self.comm_stream)
            g.replay()
            if post is not None:
                self.comm_stream.wait_stream(cur)
                with torch.cuda.stream(self.comm_stream):
                    self._post(post)

    # ----------------------------------------------------------------------------------
    def _load_images(self, images_u8: torch.Tensor, src_table, n: int, non_blocking: bool = True) -> None:
        """``n`` samples into the program's static input buffers, outside any captured graph. Dense: ``images_u8``
        [n, Hs, Ws, C]. Ragged (``src_ragged``): the packed 1-D bytes of the batch, at most the arena, and its table
        int32 [n, 4]; rows past ``n`` keep what they held."""
        p = self.prog
        if p.src_tab is None:
            if src_table is not None:
                raise ValueError("src_table belongs to a ragged trainer (src_ragged=(max_h, max_w)); this one takes "
                                 "dense [N, Hs, Ws, C] batches")
            (p.img_u8 if n == p.N else p.img_u8[:n]).copy_(images_u8, non_blocking=non_blocking)
            return
        if not isinstance(images_u8, torch.Tensor) or images_u8.dim() != 1 or images_u8.dtype != torch.uint8:
            raise ValueError(f"a ragged trainer takes the packed 1-D uint8 bytes of the batch and its src_table, got "
                             f"{getattr(images_u8, 'dtype', type(images_u8))} {tuple(getattr(images_u8, 'shape', ()))}")
        if src_table is None:
            raise ValueError("a ragged trainer needs src_table (int32 [n, 4]) with every batch of images")
        if not isinstance(src_table, torch.Tensor) or src_table.dtype != torch.int32:
            raise TypeError(f"src_table: expected an int32 tensor [{n}, 4], got "
                            f"{getattr(src_table, 'dtype', type(src_table))}")
        if tuple(src_table.shape) != (n, 4):
            raise ValueError(f"src_table: expected shape ({n}, 4), got {tuple(src_table.shape)}")
        if images_u8.numel() > p.img_u8.numel():
            raise ValueError(f"the packed batch has {images_u8.numel()} bytes, the arena of src_ragged="
                             f"{p.src_ragged} holds {p.img_u8.numel()}")
        p.img_u8[:images_u8.numel()].copy_(images_u8, non_blocking=non_blocking)
        p.src_tab[:n].copy_(src_table, non_blocking=non_blocking)

    def step(self, images_u8: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None,
             boxes: Optional[torch.Tensor] = None, flips: Optional[torch.Tensor] = None,
             src_table: Optional[torch.Tensor] = None):
        """One training step. ``images_u8`` [N,Hs,Ws,C] uint8, ``labels`` [N] int64, optional
        crop ``boxes`` [N,4] / ``flips`` [N] are copied into the program's static input buffers
        (pass None to reuse what is already there). A ragged trainer (``src_ragged``) takes the packed 1-D bytes
        of the batch as ``images_u8`` together with ``src_table`` int32 [N, 4] (data/loader.py ``pack_layout``);
        ``boxes`` are then in each sample's own coordinates."""
        if self._eval_on:
            # the BN scale / shift buffers the pass prepared once are the training forward's too
            raise RuntimeError("step() inside an evaluation pass: call eval_end() first")
        p = self.prog
        p.training = True
        if images_u8 is not None:
            self._load_images(images_u8, src_table, p.N)
        elif src_table is not None:
            raise ValueError("src_table describes the images it comes with: pass both or neither")
        if labels is not None:
            p.labels.copy_(labels, non_blocking=True)
        if boxes is not None:
            p.boxes.copy_(boxes, non_blocking=True)
        if flips is not None:
            p.flip.copy_(flips, non_blocking=True)
        if self._mix is not None:
            self._sample_mix()
        if self._drop_rng is not None:
            self._sample_drop_path()
        # gradient accumulation: every call but the window's last is a micro-step
        boundary = self.micro == self.k - 1
        self._set_hyper(boundary)
        try:
            self._step_inner(micro=not boundary)
        except BaseException:
            p.drop_pending()  # a side batch deferred by the failed step must not launch later
            raise
        self.micro = 0 if boundary else self.micro + 1
        if self.zero is not None:
            # a replayed graph does not run zero.step() in Python: keep its counter (saved in
            # ZeRO checkpoints) on the trainer's
            self.zero.step_count = self.step_count

    def _step_inner(self, micro: bool = False):
        if not self.use_graphs:
            self._run_phases_eager(micro)
            return
        if not (self.micro_graphs if micro else self.graphs):
            # two eager warm-up steps (allocator / library handles), then capture. The warm-up
            # steps are real steps: they update weights like any other. (Each step kind -- full /
            # boundary, micro -- warms up and is captured on its own.)
            warm = "_warm_micro" if micro else "_warm"
            if getattr(self, warm, 0) < 2:
                setattr(self, warm, getattr(self, warm, 0) + 1)
                self._run_phases_eager(micro)
                return
            # stream capture records without executing: no state to snapshot
            self._capture(micro)
        self._replay(micro)

    # ----------------------------------------------------------------------------------
    @torch.no_grad()
    def evaluate_batch(self, images_u8: torch.Tensor, labels: torch.Tensor,
                       boxes: Optional[torch.Tensor] = None, use_ema: Optional[bool] = None,
                       src_table: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Eval-mode forward (running BN stats); returns logits (bf16) and accumulates metrics.
        A short final batch is padded (padding rows get label -> excluded by the caller).
        ``use_ema``: evaluate the averaged weights and running statistics (None: when enabled). Nothing
        of it outlives the call: every step and every evaluation prepares its own bf16 weights."""
        p = self.prog
        use_ema = self.ema is not None if use_ema is None else bool(use_ema)
        if use_ema and self.ema is None:
            raise ValueError("use_ema=True needs a trainer built with ema_decay > 0")
        p.training = False
        if self.comm_stream is not None:  # the last step's parameter all-gather (ZeRO)
            torch.cuda.current_stream(self.dev).wait_stream(self.comm_stream)
        n = int(labels.shape[0]) if p.src_tab is not None else images_u8.shape[0]
        self._load_images(images_u8, src_table, n, non_blocking=False)
        p.labels[:n].copy_(labels)
        if boxes is not None:
            p.boxes[:n].copy_(boxes)
        p.flip.zero_()
        p.prepare_weights(src=self.ema if use_ema else None)
        p.load_input_u8(None)
        p.eval_ema = use_ema
        try:
            out = p.forward(smoothing=0.0, compute_grad=False, metrics=False)
        finally:
            p.eval_ema = False
            p.training = True
        return out[:n]

    # ----------------------------------------------------------------------------------
    # Evaluation pass: eval_begin() prepares what does not change between the batches of one pass (the
    # bf16 weights, every BN's eval coefficients: two launches), eval_step() runs augment + forward +
    # ce_eval per batch -- one graph replay, no host sync -- and eval_end() does the pass's one host read.
    @torch.no_grad()
    def eval_begin(self, use_ema: Optional[bool] = None, topk: int = 5) -> None:
        """Open an evaluation pass. ``use_ema`` as in :meth:`evaluate_batch`; the pass counts top-1 and
        top-``min(topk, num_classes)``. No ``step()`` until :meth:`eval_end`."""
        if self._eval_on:
            raise RuntimeError("eval_begin() inside an evaluation pass: call eval_end() first")
        p = self.prog
        use_ema = self.ema is not None if use_ema is None else bool(use_ema)
        if use_ema and self.ema is None:
            raise ValueError("use_ema=True needs a trainer built with ema_decay > 0")
        if int(topk) < 1:
            raise ValueError(f"topk must be >= 1, got {topk}")
        if self.comm_stream is not None:  # the last step's parameter all-gather (ZeRO)
            torch.cuda.current_stream(self.dev).wait_stream(self.comm_stream)
        p.prepare_weights(src=self.ema if use_ema else None)
        p.bn_eval_coeffs(ema=use_ema)
        self.eval_stats.zero_()
        self._eval_k = min(int(topk), p.num_classes)
        self._eval_on = True

    def _eval_forward(self) -> None:
        """Augment, stem, blocks, pool, fc, ce_eval: one chain on the current stream (the eval forward
        forks nothing). Weights and BN coefficients are eval_begin's."""
        p = self.prog
        p.training = False
        try:
            p.load_input_u8(None)
            p.forward(compute_grad=False, metrics=False, loss=False, bn_coeffs=False)
            K.ce_eval(p.logits, p.labels, self.eval_stats, self._eval_k, nvalid=self.eval_nvalid)
        finally:
            p.training = True

    def _capture_eval(self) -> None:
        release_dead_graphs(self.dev)
        s = torch.cuda.Stream(device=self.dev)
        s.wait_stream(torch.cuda.current_stream(self.dev))
        mode = "thread_local" if (dist.is_available() and dist.is_initialized()) else "global"  # (see _capture)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s, capture_error_mode=mode):
                self._eval_forward()
        torch.cuda.current_stream(self.dev).wait_stream(s)
        torch.cuda.synchronize(self.dev)
        self.eval_graph, self._eval_graph_k = g, self._eval_k

    @torch.no_grad()
    def eval_step(self, images_u8: torch.Tensor, labels: torch.Tensor, boxes: Optional[torch.Tensor] = None,
                  src_table: Optional[torch.Tensor] = None) -> None:
        """One batch of ``n <= N`` samples: copied into the static input buffers, rows past ``n`` ignored
        on the device (a ragged trainer: the packed bytes and ``src_table`` int32 [n, 4], as in :meth:`step`). Never synchronises. With graphs, a trainer's first two calls run eagerly, the third
        captures the eval forward and every later call -- of this pass or any later one, with or without
        the average -- replays that one graph (k is a kernel argument: another top-k captures again)."""
        if not self._eval_on:
            raise RuntimeError("eval_step() without eval_begin()")
        p = self.prog
        n = int(labels.shape[0]) if p.src_tab is not None else int(images_u8.shape[0])
        if not 0 < n <= p.N or labels.shape[0] != n:
            raise ValueError(f"eval_step: {n} images and {labels.shape[0]} labels for a batch of {p.N}")
        self._load_images(images_u8, src_table, n)
        p.labels[:n].copy_(labels, non_blocking=True)
        if boxes is not None:
            p.boxes[:n].copy_(boxes, non_blocking=True)
        if n != self._eval_n:
            self.eval_nvalid.fill_(n)
            self._eval_n = n
        p.flip.zero_()
        if not self.use_graphs:
            self._eval_forward()
            return
        if self.eval_graph is None or self._eval_graph_k != self._eval_k:
            if self._eval_warm < 2:
                self._eval_warm += 1
                self._eval_forward()
                return
            self.eval_graph = None
            self._capture_eval()
        self.eval_graph.replay()

    def eval_end(self) -> "EvalResult":
        """Close the pass and read its sums (the pass's one host read)."""
        if not self._eval_on:
            raise RuntimeError("eval_end() without eval_begin()")
        self._eval_on = False
        m = self.eval_stats.tolist()
        return EvalResult(loss_sum=m[0], top1=m[1], topk=m[2], count=int(m[3]), k=self._eval_k)

    def _ema_maps(self):
        """(master address, the model's parameters by name, averaged buffer by running-statistic address)."""
        if self.ema is None:
            raise ValueError("no weight EMA: the trainer was built with ema_decay=0")
        p = self.prog
        bn_of = {}
        for bn, (mean, var) in zip(p.bns, self.ema_bn_views):
            bn_of[bn.mod.running_mean.data_ptr()] = mean
            bn_of[bn.mod.running_var.data_ptr()] = var
        return p.master.data_ptr(), dict(p.model.named_parameters()), bn_of

    def ema_state_dict(self) -> dict:
        """The averaged model with the keys and shapes of ``model.state_dict()``: averaged parameters
        and BN running statistics; everything else (num_batches_tracked) copied as it is."""
        p = self.prog
        base, named, bn_of = self._ema_maps()
        out = {}
        for key, t in p.model.state_dict().items():
            if key in named:
                # the module parameter is a (possibly permuted) view of the flat master: the same view of ema
                off = (t.data_ptr() - base) // 4
                out[key] = torch.as_strided(self.ema, t.size(), t.stride(), off).clone()
            elif t.data_ptr() in bn_of and t.dtype == torch.float32:
                out[key] = bn_of[t.data_ptr()].clone()
            else:
                out[key] = t.detach().clone()
        return out

    def load_ema_state_dict(self, sd: dict) -> None:
        """Inverse of :meth:`ema_state_dict` (num_batches_tracked and other plain buffers are ignored)."""
        p = self.prog
        base, named, bn_of = self._ema_maps()
        cur = p.model.state_dict()
        missing = [k for k in cur if k not in sd]
        if missing:
            raise KeyError(f"load_ema_state_dict: missing keys {missing[:4]}{'...' if len(missing) > 4 else ''}")
        with torch.no_grad():
            for key, t in cur.items():
                if key in named:
                    off = (t.data_ptr() - base) // 4
                    torch.as_strided(self.ema, t.size(), t.stride(), off).copy_(sd[key])
                elif t.data_ptr() in bn_of and t.dtype == torch.float32:
                    bn_of[t.data_ptr()].copy_(sd[key])

    def sync_master(self) -> None:
        """Make the module's fp32 parameters (views of the flat master) complete on every rank:
        under ZeRO each rank only updates its shard (collective; call on all ranks before a
        checkpoint / state_dict)."""
        if self.zero is not None:
            if self.dev.type == "cuda" and self.comm_stream is not None:
                torch.cuda.current_stream(self.dev).wait_stream(self.comm_stream)
            self.zero.gather_master()

    def params_changed(self) -> None:
        """Call after writing the parameters from outside (checkpoint load): ZeRO re-derives its
        bf16 parameter copy from the (full) fp32 master; the weight EMA restarts from the new values."""
        if self.zero is not None:
            self.zero.refresh_param16()
        if self.ema is not None:
            self._seed_ema()

    def read_metrics(self, reset: bool = True) -> Tuple[float, float]:
        m = self.prog.metrics[:2].tolist()
        if reset:
            self.prog.metrics.zero_()
        return m[0], m[1]
