"""``train()`` / ``evaluate()``: the one training loop behind every frontend.

The reference has one copy-pasted loop per notebook with the
same shape: per-epoch train loss/accuracy, rank-0 MLflow logging, rank-0 evaluation, model
logging, checkpoints. This module implements that loop once:

* engine selection: the graph-captured native ResNet program (``engine.native_trainer``) when
  the model is a supported ResNet on a GPU, else the autograd engine (any module, CPU or GPU);
* data: any map-style dataset (sharded by ``ShardSampler``) or an MDS ``StreamingDataset``;
  native engine batches go through ``data.loader.NativeImageLoader`` (pinned uint8 + GPU aug);
* metrics: ONE packed all-reduce per epoch (loss sum, correct, count), logged on rank 0 with the
  reference's names (``train_loss``, ``train_accuracy``, ``val_loss``, ``val_accuracy``,
  ``learning_rate``); no per-step ``.item()`` host syncs (the reference does two per step);
* evaluation: sharded over ranks and reduced (the reference evaluates on rank 0 only, or on
  every rank redundantly in 03a), deterministic transforms (no train-time augmentation on val);
  loss, top-1 and top-k (``val_top{k}_accuracy``, ``eval_topk``) are summed on the device by
  ``ce_eval`` and read once per pass -- on the native engine each batch is one replay of a captured
  eval forward (``eval_graph``);
* checkpoints: ``checkpoint-{epoch}.pth.tar`` (rank 0) with full resume state; ``resume="latest"``
  continues from the newest one (used by launcher restarts);
* early stopping on validation loss with ``patience`` (`02_deepspeed/02_tiny_imagenet_deepspeed_resnet.py:289-297`,
  made rank-consistent: the stop decision is broadcast, the reference only breaks on rank 0);
* fault tolerance: heartbeat + injection points every step; non-finite loss aborts all ranks.
"""
from __future__ import annotations

import json
import math
import os
import time
from dataclasses import dataclass, field
from typing import Any, Callable, Dict, List, Optional, Tuple

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from ..config import (TrainConfig, auto_augment_options, from_deepspeed, has_param_groups, loss_options, mix_options,
                      mixes_batches, parse_duration, ragged_options, to_dict, validate_aug_repeats, validate_drop_path,
                      validate_train)
from ..models import build_model
from ..parallel import dist as ddist
from ..parallel.sampler import RepeatAugSampler, ShardSampler
from ..utils import checkpoint as ckpt
from ..utils import fault
from ..utils import mlflow_compat as mlflow
from .schedule import from_config as sched_from_config


@dataclass
class TrainResult:
    model: Any
    history: List[Dict[str, float]] = field(default_factory=list)
    run_id: Optional[str] = None
    best_val_accuracy: float = 0.0
    steps: int = 0
    images_per_sec: float = 0.0
    engine: str = ""
    resumed_epoch: int = 0   # > 0: this run resumed from the checkpoint of that epoch
    ema_state_dict: Optional[Dict[str, Any]] = None  # the averaged model (cfg.ema_decay > 0), else None


def _log(msg: str):
    if ddist.get_rank() == 0:
        print(msg, flush=True)


def _uint8_source(ds, ragged: bool = False) -> bool:
    """Can the native loader consume this dataset (fixed-size uint8 HWC + int label, or MDS)? ``ragged``: images of
    any sizes, decoded PIL images (an ``ImageFolder`` without a transform) included."""
    if hasattr(ds, "native_reader") or hasattr(ds, "shards"):
        return True
    try:
        x, _ = ds[0]
    except Exception:
        return False
    if ragged and not isinstance(x, (np.ndarray, torch.Tensor)) and hasattr(x, "size") and hasattr(x, "mode"):
        return x.mode in ("RGB", "L")
    return isinstance(x, np.ndarray) and x.dtype == np.uint8 and x.ndim == 3


def _sample_hw(ds) -> Tuple[int, int, int]:
    if hasattr(ds, "get_item"):
        it = ds.get_item(0)
        img = it["image"]
        a = np.asarray(img)
    else:
        a = np.asarray(ds[0][0])
    if a.ndim == 2:
        a = a[:, :, None]
    return a.shape[0], a.shape[1], a.shape[2]


def _collate_images(batch):
    xs, ys = zip(*batch)
    if isinstance(xs[0], torch.Tensor):
        x = torch.stack(xs)
    else:
        a = np.stack([np.asarray(v) for v in xs])
        if a.dtype == np.uint8:  # uint8 HWC -> float CHW in [0,1] (no Normalize given)
            a = a.transpose(0, 3, 1, 2).astype(np.float32) / 255.0
        x = torch.from_numpy(a)
    return x, torch.tensor(ys, dtype=torch.int64)


def _dict_collate(batch):
    xs = [b["image"] if isinstance(b, dict) else b[0] for b in batch]
    ys = [b["label"] if isinstance(b, dict) else b[1] for b in batch]
    return _collate_images(list(zip(xs, ys)))


def train_sampler(ds, aug_repeats: int = 1, **kw):
    """The training sampler of a map-style dataset: ``ShardSampler``, or with ``aug_repeats`` > 1 the
    ``RepeatAugSampler`` over the same permutation; None for a streaming dataset, which partitions itself (and
    refuses repeats: its ``epoch_indices`` are its own)."""
    r = validate_aug_repeats(aug_repeats)
    if hasattr(ds, "epoch_indices"):
        if r > 1:
            raise ValueError(f"data.aug_repeats={r} needs a map-style dataset: an MDS StreamingDataset draws its own "
                             f"epoch_indices, which the repeat sampler cannot reorder")
        return None
    return RepeatAugSampler(ds, num_repeats=r, **kw) if r > 1 else ShardSampler(ds, **kw)


def make_loader(ds: Dataset, batch_size: int, shuffle: bool, seed: int, num_workers: int = 0,
                drop_last: bool = False, pin: bool = False, aug_repeats: int = 1):
    sampler = train_sampler(ds, aug_repeats, shuffle=shuffle, seed=seed, drop_last=drop_last)
    if sampler is None:  # streaming dataset partitions itself
        return DataLoader(ds, batch_size=batch_size, num_workers=num_workers, collate_fn=_dict_collate,
                          drop_last=drop_last, pin_memory=pin), None
    return DataLoader(ds, batch_size=batch_size, sampler=sampler, num_workers=num_workers,
                      collate_fn=_collate_images, drop_last=drop_last, pin_memory=pin), sampler


class _Native:
    """Adapter: native trainer + loader behind a small common interface."""

    def __init__(self, cfg: TrainConfig, model, ds, dev, steps_per_epoch_hint: int, eval_ds=None):
        from ..data.loader import AugmentSpec, NativeImageLoader
        from ..engine.native_trainer import NativeTrainer, OptimConfig
        h, w, c = _sample_hw(ds)
        s = cfg.data.image_size
        o = cfg.optim
        # ragged batches: every sample keeps its size (h, w above are sample 0's and unread from here on)
        self.ragged = rg = ragged_options(cfg.data)
        src = dict(src_ragged=rg["ragged_max_hw"]) if rg else dict(src_hw=(h, w))
        mean = std = None
        if cfg.data.dataset in ("cifar10", "cifar"):
            from ..data.transforms import CIFAR_MEAN, CIFAR_STD
            mean, std = CIFAR_MEAN, CIFAR_STD
        from ..models.wrappers import FrozenBackboneClassifier
        ar = torch.bfloat16 if cfg.allreduce_dtype == "bf16" else torch.float32
        if isinstance(model, FrozenBackboneClassifier):
            from ..engine.frozen_trainer import FrozenFeatureTrainer
            self.tr = FrozenFeatureTrainer(model, cfg.batch_size, (s, s), dev, o,
                                           label_smoothing=cfg.data.label_smoothing, **src, mean=mean,
                                           std=std, bucket_cap_mb=cfg.bucket_cap_mb, allreduce_dtype=ar,
                                           **loss_options(cfg.data))
        else:
            self.tr = NativeTrainer(model, cfg.batch_size, (s, s), dev,
                                    optim=OptimConfig(o.name, o.lr, o.momentum, 0.0, o.nesterov, o.weight_decay,
                                                      tuple(o.betas), o.eps, o.grad_clip,
                                                      trust_coefficient=o.trust_coefficient,
                                                      adapt_1d=o.adapt_1d, trust_min=o.trust_min,
                                                      trust_max=o.trust_max, groups=list(o.groups),
                                                      norm_weight_decay=o.norm_weight_decay,
                                                      bias_weight_decay=o.bias_weight_decay),
                                    label_smoothing=cfg.data.label_smoothing, use_graphs=cfg.graphs,
                                    bucket_cap_mb=cfg.bucket_cap_mb, allreduce_dtype=ar,
                                    **src, mean=mean, std=std, zero_stage=cfg.zero.stage,
                                    seed=cfg.seed, grad_accum=cfg.grad_accum, ema_decay=cfg.ema_decay,
                                    ema_warmup=cfg.ema_warmup, **mix_options(cfg.data),
                                    **auto_augment_options(cfg.data), **loss_options(cfg.data),
                                    drop_path_rate=cfg.drop_path_rate)
        self.ema_eval = bool(cfg.ema_eval)
        self.eval_topk, self.eval_graph = _eval_topk(cfg), bool(cfg.eval_graph)
        if rg:  # torchvision's RandomResizedCrop + flip on the original image; else Resize(shorter side to s)
            aug = (AugmentSpec(mode="random_resized_crop", hflip=True) if cfg.data.augment
                   else AugmentSpec(mode="resize_center_crop", crop_frac=1.0))
        elif not cfg.data.augment:
            aug = AugmentSpec()
        elif (h, w) == (s, s) and s <= 64:
            aug = AugmentSpec(mode="random_crop", pad=4 if s == 32 else 0, hflip=True)
        elif (h, w) == (s, s):
            aug = AugmentSpec(hflip=True)
        else:
            aug = AugmentSpec(mode="random_resized_crop", hflip=True)
        sampler = train_sampler(ds, cfg.data.aug_repeats, shuffle=cfg.data.shuffle, seed=cfg.seed, drop_last=True)
        self.sampler = sampler
        self.loader = NativeImageLoader(ds, cfg.batch_size, (h, w), dev, channels=c, augment=aug, out_hw=(s, s),
                                        indices_fn=(lambda e: (sampler.set_epoch(e), sampler.indices().numpy())[1])
                                        if sampler else None, seed=cfg.seed + ddist.get_rank(),
                                        nthreads=max(1, cfg.data.num_workers), **rg)
        self.eval_spec = AugmentSpec(mode="center_crop" if (h, w) != (s, s) else "none")
        if rg:  # torchvision's Resize(s / 0.875) + CenterCrop(s), on each image's own size
            self.eval_spec = AugmentSpec(mode="resize_center_crop", crop_frac=0.875)
        self.in_hw = (h, w)
        self.batch = cfg.batch_size

    def epoch_batches(self, epoch: int):
        self.loader.set_epoch(epoch)
        return iter(self.loader)

    def steps_per_epoch(self) -> int:
        return len(self.loader)

    def step(self, batch):
        img, lab, boxes, flips = batch[:4]
        if self.ragged:
            self.tr.step(img, lab, boxes, flips, src_table=batch[4])
        else:
            self.tr.step(img, lab, boxes, flips)

    @staticmethod
    def batch_samples(batch) -> int:
        return int(batch[1].shape[0])

    def set_lr(self, lr):
        self.tr.set_lr(lr)

    def read_metrics(self):
        return self.tr.read_metrics()

    @torch.no_grad()
    def eval_dataset(self, ds) -> Tuple[float, float, float, int]:
        """(loss sum, top-1 count, top-k count, samples) of this rank's shard of ``ds``."""
        import torch.nn.functional as F
        from ..data.loader import NativeImageLoader
        from ..ops import kernels as K
        tr = self.tr
        sampler = ShardSampler(ds, shuffle=False, drop_last=False) if not hasattr(ds, "epoch_indices") else None
        h, w, c = _sample_hw(ds)
        ld = NativeImageLoader(ds, self.batch, (h, w), tr.dev, channels=c, augment=self.eval_spec,
                               out_hw=(tr.prog.H, tr.prog.W), drop_last=False,
                               indices_fn=(lambda e: sampler.indices().numpy()) if sampler else None, prefetch=1,
                               **self.ragged)
        tab = (lambda b: dict(src_table=b[4])) if self.ragged else (lambda b: {})
        has_ema = getattr(tr, "ema", None) is not None  # cfg.ema_eval: validate the averaged weights
        k = self.eval_topk  # (0: no top-k count; clipped to the class count where it is used)
        if self.eval_graph and hasattr(tr, "eval_begin"):
            # one prepared pass: a graph replay per batch, metrics on the device, one host read
            tr.eval_begin(use_ema=self.ema_eval if has_ema else None, topk=max(k, 1))  # (clips k itself)
            try:
                for b in ld:
                    tr.eval_step(b[0], b[1], b[2], **tab(b))
            finally:
                r = tr.eval_end()
            return r.loss_sum, r.top1, (r.topk if k else 0.0), r.count
        stats = torch.zeros(4, device=tr.dev, dtype=torch.float64)  # K.ce_eval's sums, read once
        frozen = not hasattr(tr, "eval_begin")  # frozen backbone: every metric from the device buffer
        loss, corr, n = 0.0, 0.0, 0
        for b in ld:
            img, lab, boxes = b[:3]
            if has_ema:
                logits = tr.evaluate_batch(img, lab, boxes, use_ema=self.ema_eval, **tab(b))
            else:
                logits = tr.evaluate_batch(img, lab, boxes, **tab(b))
            if frozen or k:
                K.ce_eval(logits.contiguous(), lab, stats, max(1, min(k, logits.shape[1])))
            if not frozen:  # eval_graph off: the host path (torch CE and argmax on the fp32 logits)
                logits = logits.float()
                loss += F.cross_entropy(logits, lab, reduction="sum").item()
                corr += (logits.argmax(1) == lab).sum().item()
                n += lab.shape[0]
        s = stats.tolist()
        if frozen:
            return s[0], s[1], (s[2] if k else 0.0), int(s[3])
        return loss, corr, (s[2] if k else 0.0), n

    @property
    def model(self):
        return getattr(self.tr, "full_model", None) or self.tr.prog.model


class _Autograd:
    def __init__(self, cfg: TrainConfig, model, ds, dev):
        from ..engine.autograd_trainer import AutogradTrainer
        self.tr = AutogradTrainer(model, dev, cfg.optim, label_smoothing=cfg.data.label_smoothing,
                                  bucket_cap_mb=cfg.bucket_cap_mb, zero_stage=cfg.zero.stage,
                                  grad_accum=cfg.grad_accum, **mix_options(cfg.data), **loss_options(cfg.data),
                                  offload_optimizer=cfg.zero.offload_optimizer, offload_param=cfg.zero.offload_param,
                                  bf16=cfg.precision == "bf16", stage3=_stage3_kw(cfg.zero),
                                  allreduce_dtype=torch.bfloat16 if cfg.allreduce_dtype == "bf16" else torch.float32)
        self.loader, self.sampler = make_loader(ds, cfg.batch_size, cfg.data.shuffle, cfg.seed,
                                                num_workers=cfg.data.num_workers if dev.type == "cuda" else 0,
                                                pin=dev.type == "cuda", aug_repeats=cfg.data.aug_repeats)
        self.batch = cfg.batch_size
        self.eval_topk = _eval_topk(cfg)

    def epoch_batches(self, epoch):
        if self.sampler is not None:
            self.sampler.set_epoch(epoch)
        elif hasattr(self.loader.dataset, "set_epoch"):
            self.loader.dataset.set_epoch(epoch)
        return iter(self.loader)

    def steps_per_epoch(self):
        return len(self.loader)

    def step(self, batch):
        self.tr.step(*batch)

    @staticmethod
    def batch_samples(batch) -> int:
        return int(batch[1].shape[0])

    def set_lr(self, lr):
        self.tr.set_lr(lr)

    def read_metrics(self):
        return self.tr.read_metrics()

    def eval_dataset(self, ds):
        """(loss sum, top-1 count, top-k count, samples): ``reference.ce_eval`` on every batch's logits into
        one device buffer, read once."""
        loader, _ = make_loader(ds, self.batch, False, 0)
        stats = torch.zeros(4, device=self.tr.dev, dtype=torch.float64)
        for x, y in loader:
            self.tr.eval_stats(x, y, stats, self.eval_topk)
        s = stats.tolist()
        return s[0], s[1], (s[2] if self.eval_topk else 0.0), int(s[3])

    @property
    def model(self):
        return self.tr.model


def _stage3_kw(z) -> Dict[str, Any]:
    """The ZeRO-3 knobs parallel/fsdp.py honours (DeepSpeed ``stage3_*`` keys)."""
    return {"persistence_threshold": z.stage3_param_persistence_threshold,
            "prefetch_elems": z.stage3_prefetch_bucket_size}


def _pick_engine(cfg: TrainConfig, model, ds, dev) -> str:
    from ..engine.program import supports
    from ..models.wrappers import FrozenBackboneClassifier
    if cfg.engine in ("native", "autograd"):
        return cfg.engine
    if cfg.zero.stage == 3 or cfg.zero.offload_optimizer or cfg.zero.offload_param:
        return "autograd"  # parameter sharding / offload: parallel/fsdp.py on the autograd engine
    if cfg.precision != "bf16":
        return "autograd"  # the native kernels compute in bf16 (fp32 master weights)
    frozen = isinstance(model, FrozenBackboneClassifier) and supports(model.resnet) and \
        not any(p.requires_grad for p in model.resnet.parameters() if p is not None and
                not any(p is q for q in model.resnet.fc.parameters()))
    # (gradient accumulation: the native trainer's micro-steps; the frozen-backbone trainer has none)
    if dev.type == "cuda" and (supports(model) or frozen) and _uint8_source(ds, bool(cfg.data.ragged)) \
            and (cfg.grad_accum == 1 or not frozen) \
            and (not mixes_batches(cfg.data) or not frozen):  # CutMix / MixUp / erasing: the native input kernel
        return "native"
    return "autograd"


def _apply_env_overrides(cfg: TrainConfig) -> TrainConfig:
    ds_json = os.environ.get("DBX_DEEPSPEED_CONFIG")
    if ds_json and not getattr(cfg, "deepspeed_applied", False):
        cfg = from_deepspeed(json.loads(ds_json), cfg)
    return cfg


def _log_param_groups(runner) -> None:
    """The distinct (weight_decay, lr_mult) groups with their parameter counts, once."""
    tr = runner.tr
    if hasattr(tr, "param_group_summary"):
        rows = tr.param_group_summary()
    else:
        rows = [(g["weight_decay"], g.get("lr_mult", 1.0), len(g["params"]), sum(p.numel() for p in g["params"]))
                for g in (tr.opt.param_groups if tr.opt is not None else [])]
    for wd, lm, nt, ne in rows:
        _log(f"[train] param group weight_decay={wd:g} lr_mult={lm:g}: {nt} tensors, {ne} parameters")


def _eval_topk(cfg: TrainConfig) -> int:
    if cfg.eval_topk < 0:
        raise ValueError(f"eval_topk must be >= 0 (0 = off), got {cfg.eval_topk}")
    return int(cfg.eval_topk)


def evaluate(runner, dataset) -> Dict[str, float]:
    """``val_loss``, ``val_accuracy``, ``val_top{k}_accuracy`` (k = ``eval_topk``, unless 0; a model with
    fewer than k classes counts top-``num_classes``) and ``val_samples``: one packed all-reduce."""
    loss, corr, topk, n = runner.eval_dataset(dataset)
    loss, corr, topk, n = ddist.all_reduce_sum([loss, corr, topk, float(n)])
    out = {"val_loss": loss / max(1.0, n), "val_accuracy": corr / max(1.0, n), "val_samples": n}
    k = getattr(runner, "eval_topk", 0)
    if k:
        out[f"val_top{k}_accuracy"] = topk / max(1.0, n)
    return out


def train(cfg: Optional[TrainConfig] = None, model: Optional[torch.nn.Module] = None,
          train_dataset: Optional[Dataset] = None, eval_dataset: Optional[Dataset] = None,
          log_mlflow: bool = True, callbacks: Optional[List[Callable]] = None, **overrides) -> TrainResult:
    """Train ``model`` (default: ``build_model(cfg.model)``) on ``train_dataset`` (default: from cfg.data)."""
    cfg = cfg or TrainConfig()
    if overrides:
        from ..config import update_dataclass
        update_dataclass(cfg, overrides)
    cfg = _apply_env_overrides(cfg)
    force_cpu = os.environ.get("DBX_FORCE_CPU") == "1"
    info = ddist.init_distributed(device="cpu" if force_cpu else None)
    dev = info.device
    torch.manual_seed(cfg.seed)
    np.random.seed(cfg.seed)
    if model is None:
        model = build_model(cfg.model, num_classes=cfg.num_classes)
    if train_dataset is None:
        from ..data.datasets import build_dataset
        d = cfg.data
        if d.dataset == "mds":
            from ..data.mds import StreamingDataset
            train_dataset = StreamingDataset(remote=d.mds_remote or None, local=d.mds_local or d.root, shuffle=d.shuffle)
        else:
            train_dataset = build_dataset(d.dataset, d.root, True, None, d.image_size, cfg.num_classes,
                                          d.train_samples or 50 * cfg.batch_size * info.world_size, cfg.seed)
    validate_train(cfg)  # (validated whichever engine runs)
    train_sampler(train_dataset, cfg.data.aug_repeats)  # (refuses repeats of a streaming dataset up front)
    engine = _pick_engine(cfg, model, train_dataset, dev)
    if validate_drop_path(cfg.drop_path_rate) > 0:  # refused, never ignored
        from ..models.wrappers import FrozenBackboneClassifier
        if engine != "native" or isinstance(model, FrozenBackboneClassifier):
            raise ValueError(f"drop_path_rate={cfg.drop_path_rate} needs the native training step (NativeTrainer, "
                             f"which gates the blocks' last BatchNorm); this run would use the "
                             f"{'frozen-backbone' if engine == 'native' else engine} engine, which drops no block")
    if cfg.data.ragged:  # refused, never ignored
        from ..models.wrappers import FrozenBackboneClassifier
        if engine != "native" or isinstance(model, FrozenBackboneClassifier):
            raise ValueError(f"data.ragged needs the native training step (NativeTrainer, whose input kernels read "
                             f"every image at its own size); this run would use the "
                             f"{'frozen-backbone' if engine == 'native' else engine} engine, which takes one dense "
                             f"batch")
    if cfg.data.auto_augment is not None:  # refused, never ignored
        from ..models.wrappers import FrozenBackboneClassifier
        if engine != "native" or isinstance(model, FrozenBackboneClassifier):
            raise ValueError(f"data.auto_augment={cfg.data.auto_augment!r} needs the native training step "
                             f"(NativeTrainer, whose input kernels apply it); this run would use the "
                             f"{'frozen-backbone' if engine == 'native' else engine} engine, which has no such "
                             f"input stage")
        in_ch = getattr(getattr(model, "conv1", None), "in_channels", 3)
        if in_ch != 3:
            raise ValueError(f"data.auto_augment={cfg.data.auto_augment!r} needs 3-channel images, the model "
                             f"takes {in_ch}")
    if not 0.0 <= cfg.ema_decay < 1.0:
        raise ValueError(f"ema_decay must be in [0, 1), got {cfg.ema_decay}")
    if cfg.ema_decay > 0:
        from ..models.wrappers import FrozenBackboneClassifier
        if engine != "native" or isinstance(model, FrozenBackboneClassifier):
            raise ValueError("ema_decay > 0 needs the native training step (NativeTrainer); this run would use the "
                             f"{'frozen-backbone' if engine == 'native' else engine} engine, which keeps no weight EMA")
    if has_param_groups(cfg.optim):
        from ..models.wrappers import FrozenBackboneClassifier
        if engine == "native" and isinstance(model, FrozenBackboneClassifier):
            raise ValueError("parameter groups (optim.groups / norm_weight_decay / bias_weight_decay) are not "
                             "supported by the frozen-backbone trainer this run would use: only the head trains")
    runner = _Native(cfg, model, train_dataset, dev, 0) if engine == "native" else _Autograd(cfg, model, train_dataset, dev)
    spe = runner.steps_per_epoch()
    total = cfg.max_steps or (parse_duration(cfg.duration, spe, cfg.batch_size) if cfg.duration else spe * cfg.epochs)
    epochs = math.ceil(total / max(1, spe))
    sched = sched_from_config(cfg.sched, cfg.optim.lr, total, spe)
    res = TrainResult(model=model, engine=engine)
    from ..parallel import comm_guard
    watchdog = comm_guard.for_runner(runner, dev)  # a hung / failed peer ends this rank (launcher restarts)
    try:
        # --- resume ----------------------------------------------------------------------------
        start_epoch, step = 0, 0
        if cfg.checkpoint_dir and (cfg.resume == "latest" or int(os.environ.get("DBX_RESTART_COUNT", "0")) > 0):
            path = ckpt.latest_checkpoint(cfg.checkpoint_dir)
            if path:
                st = torch.load(path, map_location="cpu", weights_only=True)
                model.load_state_dict(st["model"])
                _params_changed(runner)
                _restore_trainer_state(runner, st.get("trainer"))
                start_epoch, step = int(st.get("epoch", 0)), int(st.get("step", 0))
                _restore_shard_state(runner, cfg.checkpoint_dir, start_epoch)
                res.history = list(st.get("history", []))
                res.resumed_epoch = start_epoch
                _log(f"[train] resumed from {path} (epoch {start_epoch}, step {step})")
        elif cfg.resume and cfg.resume != "latest":
            st = torch.load(cfg.resume, map_location="cpu", weights_only=True)
            model.load_state_dict(st["model"])
            _params_changed(runner)
        # --- mlflow ------------------------------------------------------------------------------
        is_main = ddist.get_rank() == 0
        if is_main and log_mlflow:
            mlflow.set_experiment(cfg.experiment)
            run = mlflow.start_run(run_name=cfg.run_name or None, nested=mlflow.active_run() is not None)
            res.run_id = run.info.run_id
            mlflow.log_params({"batch_size": cfg.batch_size, "epochs": epochs, "learning_rate": cfg.optim.lr,
                               "model_type": cfg.model, "optimizer": cfg.optim.name, "weight_decay": cfg.optim.weight_decay,
                               "scheduler": cfg.sched.name, "num_gpus": ddist.get_world_size(), "engine": engine,
                               "zero_stage": cfg.zero.stage, "trainer": "dbx_amd", "ema_decay": cfg.ema_decay})
        _log(f"[train] engine={engine} world={ddist.get_world_size()} steps/epoch={spe} total_steps={total}")
        if has_param_groups(cfg.optim):
            _log_param_groups(runner)
        if mixes_batches(cfg.data) or cfg.data.auto_augment is not None:
            s = runner.tr.mix_summary() if hasattr(runner.tr, "mix_summary") else mix_options(cfg.data)
            _log("[train] batch mixing: " + " ".join(f"{k}={v}" for k, v in s.items()))
        if cfg.data.loss != "ce":
            s = runner.tr.loss_summary() if hasattr(runner.tr, "loss_summary") else loss_options(cfg.data)
            _log("[train] training loss: " + " ".join(f"{k}={v}" for k, v in s.items())
                 + " (validation reports softmax cross-entropy)")
        if cfg.drop_path_rate > 0:
            _log("[train] stochastic depth: " + " ".join(f"{k}={v}" for k, v in runner.tr.drop_path_summary().items())
                 + " (whole blocks per micro-batch and rank; evaluation is never gated)")
        if cfg.data.aug_repeats > 1:
            _log(f"[train] repeated augmentation: aug_repeats={cfg.data.aug_repeats} sampler="
                 f"{type(runner.sampler).__name__} (an epoch keeps its length and visits about "
                 f"1/{cfg.data.aug_repeats} of the images; validation never repeats)")
        if cfg.grad_accum > 1 and cfg.checkpoint_dir and cfg.checkpoint_every and spe % cfg.grad_accum != 0:
            # (one iteration is one micro-batch; a checkpoint carries no accumulator)
            _log(f"[train] warning: steps/epoch={spe} is no multiple of grad_accum={cfg.grad_accum}: a run resumed "
                 "from an epoch checkpoint drops the micro-batches of the window that was open at that epoch's end")
        best_val, bad_epochs = -1.0, 0
        t_start = time.perf_counter()
        imgs = 0
        stop = False
        for epoch in range(start_epoch, epochs):
            t0 = time.perf_counter()
            n_local = 0  # samples actually stepped this epoch (early stop / short final batch)
            t_wait = t_wall = 0.0  # wall_clock_breakdown: host time waiting for batches / per logging window
            t_mark = time.perf_counter()
            n_win = 0
            it = iter(runner.epoch_batches(epoch))
            while step < total:
                t_b = time.perf_counter()
                batch = next(it, None)
                if batch is None:
                    break
                t_wait += time.perf_counter() - t_b
                runner.set_lr(sched(step))
                fault.heartbeat(step)
                if fault.maybe_inject(step):
                    raise FloatingPointError(f"injected NaN loss at step {step}")
                if watchdog is not None:
                    watchdog.step_begin(step)
                runner.step(batch)
                if watchdog is not None:
                    watchdog.step_end()
                step += 1
                n_win += 1
                n_local += runner.batch_samples(batch)
                imgs += cfg.batch_size * ddist.get_world_size()
                if cfg.log_every and step % cfg.log_every == 0:
                    if cfg.wall_clock_breakdown:  # DeepSpeed's per-window timing (synchronised at the window end)
                        if dev.type == "cuda":
                            torch.cuda.synchronize()
                        t_wall = time.perf_counter() - t_mark
                        if is_main:
                            print(f"[wall_clock_breakdown] steps {step - n_win + 1}-{step}: "
                                  f"{1e3 * t_wall / n_win:.2f} ms/step, data wait {1e3 * t_wait / n_win:.2f} ms/step, "
                                  f"compute+sync {1e3 * (t_wall - t_wait) / n_win:.2f} ms/step", flush=True)
                        t_wait, n_win, t_mark = 0.0, 0, time.perf_counter()
                    if is_main:
                        print(f"[TRAINING] [RANK {ddist.get_rank()}] step {step}/{total} (epoch {epoch + 1})", flush=True)
            if watchdog is not None:
                watchdog.step_begin(step)  # the epoch-end collectives are bounded too
            loss_sum, correct = runner.read_metrics()
            loss_sum, correct, n = ddist.all_reduce_sum([loss_sum, correct, float(n_local)])
            if watchdog is not None:
                watchdog.step_end()
            if not fault.check_finite(loss_sum):
                raise FloatingPointError(f"non-finite training loss in epoch {epoch + 1}")
            rec = {"epoch": epoch + 1, "train_loss": loss_sum / max(1.0, n), "train_accuracy": correct / max(1.0, n),
                   "learning_rate": sched(max(0, step - 1)), "epoch_time_s": time.perf_counter() - t0}
            if eval_dataset is not None and cfg.eval_every and (epoch + 1) % cfg.eval_every == 0:
                rec.update(evaluate(runner, eval_dataset))
            res.history.append(rec)
            if is_main:
                _log(f"Epoch [{epoch + 1}/{epochs}], Loss: {rec['train_loss']:.4f}, Accuracy: {rec['train_accuracy']:.4f}"
                     + (f", Val Loss: {rec['val_loss']:.4f}, Val Accuracy: {rec['val_accuracy']:.4f}" if "val_loss" in rec else ""))
                if log_mlflow:
                    mlflow.log_metrics({k: v for k, v in rec.items() if k != "epoch"}, step=epoch + 1)
            for cb in callbacks or []:
                cb(epoch + 1, rec, runner)
            if cfg.checkpoint_dir and cfg.checkpoint_every and (epoch + 1) % cfg.checkpoint_every == 0:
                _sync_master(runner)  # every rank (collective): ZeRO shards -> full fp32 parameters
                _save_shard_state(runner, cfg.checkpoint_dir, epoch + 1)  # every rank: its ZeRO shard
            if cfg.checkpoint_dir and is_main and cfg.checkpoint_every and (epoch + 1) % cfg.checkpoint_every == 0:
                ckpt.save_checkpoint(cfg.checkpoint_dir, runner.model, None, epoch + 1, step=step,
                                     trainer=_trainer_state(runner), history=res.history, config=json.dumps(to_dict(cfg)))
            ddist.barrier()
            if "val_accuracy" in rec:
                res.best_val_accuracy = max(res.best_val_accuracy, rec["val_accuracy"])
                if cfg.patience:
                    if rec["val_accuracy"] > best_val:
                        best_val, bad_epochs = rec["val_accuracy"], 0
                    else:
                        bad_epochs += 1
                    stop = bool(ddist.broadcast_object(bad_epochs >= cfg.patience))
            if stop:
                _log(f"[train] early stopping after epoch {epoch + 1} (patience {cfg.patience})")
                break
            if step >= total:
                break
        if torch.cuda.is_available() and dev.type == "cuda":
            torch.cuda.synchronize()
    finally:
        # every exit (an exception out of a step included): a live watchdog would otherwise end the
        # process DBX_COMM_TIMEOUT seconds later, under a caller that caught the exception
        if watchdog is not None:
            watchdog.close()
    el = time.perf_counter() - t_start
    _sync_master(runner)  # the returned / logged model holds the full parameters on every rank
    res.steps = step
    res.images_per_sec = imgs / el if el > 0 else 0.0
    res.model = runner.model
    if getattr(runner.tr, "ema", None) is not None:
        res.ema_state_dict = {k: v.cpu() for k, v in runner.tr.ema_state_dict().items()}
    if is_main and log_mlflow:
        mlflow.log_metric("images_per_sec", res.images_per_sec)
        mlflow.pytorch.log_model(res.model, cfg.model_name or "model")
        mlflow.log_dict({"history": res.history}, "training_history.json")
        mlflow.end_run()
    return res


def _sync_master(runner) -> None:
    f = getattr(runner.tr, "sync_master", None)
    if f is not None:
        f()


def _params_changed(runner) -> None:
    f = getattr(runner.tr, "params_changed", None)
    if f is not None:
        f()


def _trainer_state(runner) -> Dict[str, Any]:
    tr = runner.tr
    if hasattr(tr, "prog") and hasattr(tr, "mom"):  # native: flat optimizer state
        st = {"kind": "native", "mom": tr.mom.detach().cpu(), "step_count": tr.step_count}
        if tr.mom2 is not None:
            st["mom2"] = tr.mom2.detach().cpu()
        if getattr(tr, "ema", None) is not None:
            st["ema"], st["ema_bn"] = tr.ema.detach().cpu(), tr.ema_bn.detach().cpu()
        return st
    if getattr(tr, "opt", None) is not None:
        return {"kind": "torch", "optimizer": ckpt.clean_state_dict(tr.opt.state_dict())}
    return {}


def _shard_path(d: str, epoch: int) -> str:
    return os.path.join(d, f"zero_shard-{epoch}-rank{ddist.get_rank()}-of{ddist.get_world_size()}.pt")


def _sharded(runner):
    """(save, load) of this rank's sharded optimizer state (ZeRO-1/2 or ZeRO-3), if any."""
    tr = runner.tr
    if getattr(tr, "sharded", False):
        return tr.ddp.optim_state_dict, tr.ddp.load_optim_state_dict
    z = getattr(tr, "zero", None)
    if z is not None:
        return z.state_dict, z.load_state_dict
    return None


def _save_shard_state(runner, d: str, epoch: int) -> None:
    sh = _sharded(runner)
    if sh is None:
        return
    os.makedirs(d, exist_ok=True)
    torch.save(sh[0](), _shard_path(d, epoch))


def _restore_shard_state(runner, d: str, epoch: int) -> None:
    """Each rank reloads its own optimizer shard (the rank-0 checkpoint holds only rank 0's)."""
    sh = _sharded(runner)
    if sh is None:
        return
    p = _shard_path(d, epoch)
    if not os.path.exists(p):
        _log(f"[train] warning: no optimizer shard {p}; sharded optimizer state starts fresh")
        return
    sh[1](torch.load(p, map_location="cpu", weights_only=True))


def _restore_trainer_state(runner, st):
    if not st:
        return
    tr = runner.tr
    if st.get("kind") == "native" and hasattr(tr, "mom"):
        tr.mom.copy_(st["mom"])
        if "mom2" in st and tr.mom2 is not None:
            tr.mom2.copy_(st["mom2"])
        tr.step_count = int(st.get("step_count", 0))
        if hasattr(tr, "micro"):
            tr.micro = 0  # no accumulator is saved: a partial window is dropped, the next call opens one
        if getattr(tr, "ema", None) is not None:
            if "ema" in st and "ema_bn" in st:
                tr.ema.copy_(st["ema"])
                tr.ema_bn.copy_(st["ema_bn"])
            else:  # written without the average: it restarts from the loaded parameters (params_changed)
                _log("[train] warning: the checkpoint carries no weight EMA; the average is re-seeded from "
                     "the loaded parameters")
    elif st.get("kind") == "torch" and getattr(tr, "opt", None) is not None:
        tr.opt.load_state_dict(st["optimizer"])
