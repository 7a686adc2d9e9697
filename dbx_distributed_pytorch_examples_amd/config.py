"""Typed configuration: one dataclass tree, loadable from YAML/JSON/dicts with ``a.b=c`` overrides.

Replaces the reference's scattered configuration:

* ``local_config.yaml`` keys (`/root/reference/UPDATE_local_config.yaml:1-7`, read by
  `setup/00_setup.py:7-23`): ``catalog, schema, num_nodes, secret_scope, secret_key,
  cifar_cache, tiny_imagenet_cache, imagenet1k_cache, coco_cache`` -> :class:`LocalConfig`
  (Unity-Catalog volumes become local directories under ``volume_root``);
* per-file hyper-parameter constants (§2.3) -> :class:`TrainConfig`;
* DeepSpeed JSON dicts (`02_deepspeed/deepspeed_config.py`) -> :func:`from_deepspeed`;
* Composer duration strings ``"2ep"`` / ``"100ba"`` (`03_composer/01_cifar_composer_resnet.ipynb:287`)
  -> :func:`parse_duration`.
"""
from __future__ import annotations

import copy
import dataclasses
import fnmatch
import json
import math
import os
import re
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import yaml


@dataclass
class LocalConfig:
    """The reference's local_config.yaml (template `UPDATE_local_config.yaml:1-7` + `coco_cache`)."""
    catalog: str = ""
    schema: str = ""
    num_nodes: int = 1
    secret_scope: str = ""
    secret_key: str = ""
    cifar_cache: str = "cifar"
    tiny_imagenet_cache: str = "tiny_imagenet"
    imagenet1k_cache: str = "imagenet_1k"
    coco_cache: str = "ms_coco"
    volume_root: str = os.environ.get("DBX_VOLUME_ROOT", os.path.expanduser("~/.dbx_amd/volumes"))

    def volume(self, name: str) -> str:
        """Map a UC volume path (``/Volumes/<cat>/<schema>/<vol>``) or bare name to a local dir."""
        v = getattr(self, name, name)
        if v.startswith("/Volumes/"):
            v = v[len("/Volumes/"):]
        path = v if os.path.isabs(v) else os.path.join(self.volume_root, self.catalog or "main",
                                                        self.schema or "default", v)
        return path


@dataclass
class OptimizerConfig:
    name: str = "sgd"                  # sgd | adam | adamw | lars | lamb
    lr: float = 0.1
    momentum: float = 0.9
    nesterov: bool = False
    weight_decay: float = 5e-5
    betas: Tuple[float, float] = (0.9, 0.999)
    eps: float = 1e-8
    grad_clip: float = 0.0
    trust_coefficient: float = 0.001   # LARS eta
    adapt_1d: bool = False             # LAMB: also decay and adapt BN affine parameters and biases
    trust_min: float = 0.0             # LAMB trust-ratio clamp where adapted (0 = unbounded)
    trust_max: float = 0.0
    # parameter groups (sgd | adam | adamw; see resolve_param_groups)
    groups: list = field(default_factory=list)  # [{match: "layer4.*" | [patterns], weight_decay: float?, lr_mult: float?}, ...]
    norm_weight_decay: float = -1.0    # < 0: use weight_decay. Applies to every parameter of a normalisation layer
    bias_weight_decay: float = -1.0    # < 0: use weight_decay. Applies to biases of all other layers (fc.bias)


@dataclass
class SchedulerConfig:
    name: str = "none"                 # none | cosine | warmup_linear | warmup_cosine | step | warmup_lr
    warmup_steps: int = 0
    warmup_min_lr: float = 0.0
    warmup_type: str = "log"           # DeepSpeed WarmupLR: "log" (its default) | "linear"
    total_steps: int = 0
    t_max_epochs: int = 0              # CosineAnnealingLR(T_max=epochs), per-epoch stepping
    step_size: int = 30
    gamma: float = 0.1


@dataclass
class ZeroConfig:
    stage: int = 0                     # 0 = plain DDP, 1 = sharded optimizer state, 2 = + sharded grads, 3 = + sharded params
    reduce_bucket_size: int = 500_000_000
    allgather_bucket_size: int = 500_000_000
    overlap_comm: bool = True
    contiguous_gradients: bool = True
    reduce_scatter: bool = True
    offload_optimizer: bool = False    # fp32 master shard + moments in pinned host memory, CPU step (stage 3 path)
    offload_param: bool = False        # + no persistent device parameter shard
    allgather_partitions: bool = True
    sub_group_size: int = 1_000_000_000
    # stage 3 (parallel/fsdp.py): parameters smaller than the persistence threshold stay replicated
    # (never gathered / released); the prefetch size bounds how many parameter elements the next units'
    # all-gathers may run ahead of the forward; live / reuse distance are recorded (DeepSpeed
    # memory-pressure knobs with no effect at ResNet sizes on 288 GB HBM)
    stage3_prefetch_bucket_size: int = 50_000_000
    stage3_param_persistence_threshold: int = 100_000
    stage3_max_live_parameters: int = 1_000_000_000
    stage3_max_reuse_distance: int = 1_000_000_000
    stage3_gather_16bit_weights_on_model_save: bool = False


@dataclass
class DataConfig:
    dataset: str = "synthetic"         # synthetic | cifar10 | mnist | fashion_mnist | tiny_imagenet | imagenet | mds | folder | hf
    root: str = ""
    image_size: int = 224
    num_classes: int = 1000
    train_samples: int = 0             # synthetic: samples per epoch (0 = 50 batches)
    augment: bool = True
    num_workers: int = 4
    mds_remote: str = ""
    mds_local: str = ""
    shuffle: bool = True
    label_smoothing: float = 0.0
    # the training loss on the (mixed, smoothed) targets: softmax cross-entropy, or timm's binary cross-entropy on
    # the logits ("ResNet strikes back"); validation reports softmax CE and top-k under either
    loss: str = "ce"                   # ce | bce
    bce_target_threshold: Optional[float] = None  # bce: targets become t > threshold ? 1 : 0 (in [0, 1); None = soft)
    bce_sum_classes: bool = False      # bce: the sample loss is the sum over the classes, not their mean
    cutmix_alpha: float = 0.0
    # batch mixing and erasing (engine/mix.py; torchvision's ResNet-50 recipe: mixup 0.2, cutmix 1.0, erase 0.1)
    mixup_alpha: float = 0.0           # MixUp: lam ~ Beta(a, a); 0 = off
    mix_prob: float = 1.0              # a step mixes (MixUp or CutMix) with this probability
    mix_switch_prob: float = 0.5       # with both alphas > 0: the share of mixing steps that use CutMix
    erase_prob: float = 0.0            # random erasing: the share of samples that get a rectangle
    erase_mode: str = "const"          # const (0 after normalisation) | pixel (N(0, 1) per pixel and channel)
    erase_scale: Tuple[float, float] = (0.02, 1 / 3)   # rectangle area / image area
    erase_ratio: Tuple[float, float] = (0.3, 3.3)      # rectangle height / width (log-uniform)
    # TrivialAugmentWide in the native input kernels (torchvision's --auto-augment ta_wide): one of fourteen
    # uint8-space operations per training image, at one of ta_num_bins strengths. Native engine only.
    # "ra": RandAugment (torchvision's --auto-augment ra; timm's A1-A3 recipes), ra_num_ops operations in sequence at
    # bin ra_magnitude of ta_num_bins. "aa_imagenet": AutoAugment's ImageNet policy (two operations on ten bins;
    # ta_num_bins is ignored for it). The ra_* options need auto_augment: ra.
    auto_augment: Optional[str] = None  # None | "ta_wide" | "ra" | "aa_imagenet"
    ta_num_bins: int = 31
    ra_num_ops: int = 2
    ra_magnitude: int = 9
    # repeated augmentation (DeiT / timm's RepeatAugSampler; A1 / A2 use 3): every drawn image appears aug_repeats
    # times in a row in the epoch's order, each copy augmented on its own; the epoch keeps its length, so it visits
    # about 1 / aug_repeats of the images. Map-style datasets only; validation never repeats.
    aug_repeats: int = 1
    # ragged input batches (native engine): the images keep the sizes they were written with, up to ragged_max_hw
    # (height, width); a batch is one byte arena and a table, and the GPU crops every sample from its own geometry
    # (RandomResizedCrop draws on the original image). ragged_oversize: error | crop (cut around the centre).
    ragged: bool = False
    ragged_max_hw: Tuple[int, int] = (512, 512)
    ragged_oversize: str = "error"


RAGGED_OVERSIZE = ("error", "crop")


def ragged_options(d: DataConfig) -> Dict[str, Any]:
    """The loader's ``ragged_max_hw`` / ``oversize`` from ``cfg.data``, validated; ``{}`` while ``ragged`` is off
    (ValueError: a ``ragged_*`` option away from its default then -- refused, never ignored)."""
    if not isinstance(d.ragged, bool):
        raise ValueError(f"data.ragged must be a bool, got {d.ragged!r}")
    hw = tuple(d.ragged_max_hw) if isinstance(d.ragged_max_hw, (list, tuple)) else d.ragged_max_hw
    if (not isinstance(hw, tuple) or len(hw) != 2
            or any(isinstance(v, bool) or not isinstance(v, int) or v < 1 for v in hw)):
        raise ValueError(f"data.ragged_max_hw must be two integers >= 1 (height, width), got {d.ragged_max_hw!r}")
    if d.ragged_oversize not in RAGGED_OVERSIZE:
        raise ValueError(f"data.ragged_oversize must be one of {RAGGED_OVERSIZE}, got {d.ragged_oversize!r}")
    if not d.ragged:
        if hw != (512, 512) or d.ragged_oversize != "error":
            raise ValueError("data.ragged_max_hw / data.ragged_oversize need data.ragged: true")
        return {}
    return dict(ragged_max_hw=hw, oversize=d.ragged_oversize)


def mix_options(d: DataConfig) -> Dict[str, Any]:
    """The trainers' batch-mixing arguments from ``cfg.data``, validated (ValueError: a negative alpha, a
    probability outside [0, 1], an unknown erase mode, a bad scale or ratio pair)."""
    from .engine.mix import validate_mix
    kw = dict(mixup_alpha=d.mixup_alpha, cutmix_alpha=d.cutmix_alpha, mix_prob=d.mix_prob,
              mix_switch_prob=d.mix_switch_prob, erase_prob=d.erase_prob, erase_mode=d.erase_mode,
              erase_scale=d.erase_scale, erase_ratio=d.erase_ratio)
    validate_mix(**kw)
    return kw


def mixes_batches(d: DataConfig) -> bool:
    return d.cutmix_alpha > 0 or d.mixup_alpha > 0 or d.erase_prob > 0


def auto_augment_options(d: DataConfig) -> Dict[str, Any]:
    """The native trainer's ``auto_augment`` / ``ta_num_bins`` / ``ra_num_ops`` / ``ra_magnitude`` from
    ``cfg.data``, validated (ValueError: an unknown policy name, fewer than two bins, ``ra_num_ops`` outside 1..4,
    ``ra_magnitude`` outside [0, ta_num_bins), an ``ra_*`` option set while the policy is not ``ra``). The two
    ``ra_*`` arguments are passed with ``ra`` only: elsewhere they are at their defaults, or this raised."""
    from .engine.mix import validate_auto_augment
    validate_auto_augment(d.auto_augment, d.ta_num_bins, d.ra_num_ops, d.ra_magnitude)
    kw = dict(auto_augment=d.auto_augment, ta_num_bins=d.ta_num_bins)
    if d.auto_augment == "ra":
        kw.update(ra_num_ops=d.ra_num_ops, ra_magnitude=d.ra_magnitude)
    return kw


LOSSES = ("ce", "bce")


def validate_loss(loss: Any = "ce", bce_target_threshold: Any = None, bce_sum_classes: Any = False) -> None:
    """ValueError for an unknown training loss, a ``bce_target_threshold`` outside [0, 1), or a ``bce_*``
    option while the loss is not ``bce`` (refused, never ignored). Shared by the config and the trainers."""
    if loss not in LOSSES:
        raise ValueError(f"unknown training loss {loss!r} (known: {', '.join(LOSSES)})")
    thr = bce_target_threshold
    if thr is not None:
        if isinstance(thr, bool) or not isinstance(thr, (int, float)) or not 0.0 <= float(thr) < 1.0:
            raise ValueError(f"bce_target_threshold must be a number in [0, 1) or None, got {thr!r}")
    if not isinstance(bce_sum_classes, bool):
        raise ValueError(f"bce_sum_classes must be a bool, got {bce_sum_classes!r}")
    if loss != "bce" and (thr is not None or bce_sum_classes):
        raise ValueError(f"bce_target_threshold / bce_sum_classes need loss='bce', the loss is {loss!r}")


def loss_options(d: DataConfig) -> Dict[str, Any]:
    """The trainers' training-loss arguments from ``cfg.data``, validated (:func:`validate_loss`)."""
    kw = dict(loss=d.loss, bce_target_threshold=d.bce_target_threshold, bce_sum_classes=d.bce_sum_classes)
    validate_loss(**kw)
    return kw


def validate_aug_repeats(aug_repeats: Any) -> int:
    """ValueError unless ``aug_repeats`` is an integer >= 1 (refused, never ignored)."""
    r = aug_repeats
    if isinstance(r, bool) or not isinstance(r, int) or r < 1:
        raise ValueError(f"aug_repeats must be an integer >= 1, got {r!r}")
    return r


def validate_data(d: DataConfig) -> None:
    """ValueError for a bad batch-mixing, erasing, auto-augment, training-loss or repeated-augmentation setting,
    whichever engine would run."""
    mix_options(d)
    auto_augment_options(d)
    loss_options(d)
    validate_aug_repeats(d.aug_repeats)
    ragged_options(d)


def validate_drop_path(rate: Any) -> float:
    """ValueError unless the stochastic-depth rate is a number in [0, 1). Shared by the config and the trainers."""
    if isinstance(rate, bool) or not isinstance(rate, (int, float)) or not 0.0 <= float(rate) < 1.0:
        raise ValueError(f"drop_path_rate must be a number in [0, 1), got {rate!r}")
    return float(rate)


def drop_path_probs(rate: float, nblocks: int) -> List[float]:
    """timm's linear stochastic-depth rule over ``nblocks`` residual blocks: p_l = rate * l / (L - 1), in
    float64 (Python floats). The first block is never dropped, the last one with probability ``rate``."""
    rate = validate_drop_path(rate)
    if nblocks < 1:
        raise ValueError(f"drop_path_probs: {nblocks} blocks")
    if nblocks == 1:
        return [0.0]
    return [rate * l / (nblocks - 1) for l in range(nblocks)]


def validate_train(cfg: "TrainConfig") -> None:
    """ValueError for a bad data setting (:func:`validate_data`) or stochastic-depth rate."""
    validate_data(cfg.data)
    validate_drop_path(cfg.drop_path_rate)


@dataclass
class TrainConfig:
    model: str = "resnet50"
    num_classes: int = 1000
    batch_size: int = 256              # per GPU (micro batch)
    grad_accum: int = 1
    ema_decay: float = 0.0             # weight EMA (native engine): 0 = off, else the decay d in [0, 1)
    ema_warmup: bool = False           # d_t = min(ema_decay, (1 + t) / (10 + t)) at optimizer step t
    ema_eval: bool = True              # val_* metrics from the averaged weights when ema_decay > 0
    # stochastic depth, per batch (native engine): block l of L is dropped for a whole micro-batch with probability
    # rate * l / (L - 1) and scaled by 1 / (1 - p_l) otherwise (timm's linear rule; A1 / A2 use 0.05). In [0, 1).
    drop_path_rate: float = 0.0
    epochs: int = 1
    max_steps: int = 0                 # 0 = full epochs
    duration: str = ""                 # composer style: "2ep" / "100ba"
    seed: int = 42
    precision: str = "bf16"
    engine: str = "auto"               # auto | native | autograd
    graphs: bool = True
    bucket_cap_mb: float = 64.0
    allreduce_dtype: str = "fp32"
    log_every: int = 100
    eval_every: int = 1
    eval_topk: int = 5                 # val_top{k}_accuracy next to val_accuracy (0 = off; k is clipped to num_classes)
    eval_graph: bool = True            # native engine: validation as one captured graph with device-side metrics
    patience: int = 0                  # early stopping (02_tiny_imagenet_deepspeed_resnet.py:289-297)
    checkpoint_dir: str = ""
    checkpoint_every: int = 1
    resume: str = ""                   # path or "latest"
    experiment: str = "dbx_amd"
    run_name: str = ""
    model_name: str = "model"          # MLflow model artifact name (the notebooks' per-file names)
    wall_clock_breakdown: bool = False # DeepSpeed wall_clock_breakdown: per-phase timers (utils/profiling.py)
    tensorboard_dir: str = ""          # DeepSpeed tensorboard.output_path when enabled (recorded; MLflow is the sink)
    optim: OptimizerConfig = field(default_factory=OptimizerConfig)
    sched: SchedulerConfig = field(default_factory=SchedulerConfig)
    zero: ZeroConfig = field(default_factory=ZeroConfig)
    data: DataConfig = field(default_factory=DataConfig)
    local: LocalConfig = field(default_factory=LocalConfig)


# ----------------------------------------------------------------------------------------
def _coerce(cur: Any, val: Any) -> Any:
    if isinstance(cur, bool):
        if isinstance(val, str):
            return val.lower() in ("1", "true", "yes", "on")
        return bool(val)
    if isinstance(cur, int) and not isinstance(cur, bool):
        return int(float(val)) if isinstance(val, str) else int(val)
    if isinstance(cur, float):
        return float(val)
    if isinstance(cur, tuple):
        if isinstance(val, str):
            val = [float(x) for x in val.strip("()[]").split(",")]
        return tuple(type(c)(v) for c, v in zip(cur, val))
    if isinstance(cur, list):
        if isinstance(val, str):  # a CLI override: optim.groups='[{"match": "fc.*", "lr_mult": 10}]'
            val = json.loads(val)
        if not isinstance(val, (list, tuple)):
            raise ValueError(f"expected a list, got {val!r}")
        return list(val)
    return val


def update_dataclass(obj: Any, d: Dict[str, Any], strict: bool = True) -> Any:
    for k, v in d.items():
        if not hasattr(obj, k):
            if strict:
                raise KeyError(f"unknown config key {k!r} for {type(obj).__name__}")
            continue
        cur = getattr(obj, k)
        if dataclasses.is_dataclass(cur) and isinstance(v, dict):
            update_dataclass(cur, v, strict)
        else:
            setattr(obj, k, _coerce(cur, v) if cur is not None else v)
    return obj


def apply_overrides(cfg: Any, overrides: Sequence[str]) -> Any:
    """CLI overrides ``a.b=c`` (values parsed as YAML scalars)."""
    for ov in overrides:
        if "=" not in ov:
            raise ValueError(f"override {ov!r} is not key=value")
        key, val = ov.split("=", 1)
        parts = key.split(".")
        obj = cfg
        for p in parts[:-1]:
            obj = getattr(obj, p)
        if not hasattr(obj, parts[-1]):
            raise KeyError(f"unknown config key {key!r}")
        cur = getattr(obj, parts[-1])
        parsed = yaml.safe_load(val)
        setattr(obj, parts[-1], _coerce(cur, parsed) if cur is not None else parsed)
    return cfg


def load_config(path: Optional[str] = None, overrides: Sequence[str] = (), base: Optional[TrainConfig] = None
                ) -> TrainConfig:
    cfg = copy.deepcopy(base) if base is not None else TrainConfig()
    if path:
        with open(path) as f:
            d = json.load(f) if path.endswith(".json") else yaml.safe_load(f)
        d = d or {}
        if "train_micro_batch_size_per_gpu" in d or "zero_optimization" in d:
            cfg = from_deepspeed(d, cfg)
        elif set(d) & set(f.name for f in dataclasses.fields(LocalConfig)) and not set(d) & {"model", "optim"}:
            update_dataclass(cfg.local, d, strict=False)
        else:
            update_dataclass(cfg, d)
    return apply_overrides(cfg, overrides)


def load_local_config(path: str = "../local_config.yaml") -> LocalConfig:
    """``setup/00_setup.py:9-23`` equivalent; missing file -> defaults."""
    lc = LocalConfig()
    if os.path.exists(path):
        with open(path) as f:
            update_dataclass(lc, yaml.safe_load(f) or {}, strict=False)
    return lc


def to_dict(cfg: Any) -> Dict[str, Any]:
    return dataclasses.asdict(cfg)


# ----------------------------------------------------------------------------------------
_GROUP_KEYS = ("match", "weight_decay", "lr_mult")


def has_param_groups(optim: Any) -> bool:
    """Whether ``optim`` sets any per-parameter-group field (``groups`` or one of the two shorthands)."""
    return bool(getattr(optim, "groups", None)) or float(getattr(optim, "norm_weight_decay", -1.0)) >= 0 \
        or float(getattr(optim, "bias_weight_decay", -1.0)) >= 0 \
        or any(math.isnan(float(getattr(optim, k, -1.0))) for k in ("norm_weight_decay", "bias_weight_decay"))


def reject_param_groups(optim: Any, who: str) -> None:
    """For the engines and optimizers that keep one weight decay and one lr: refuse, never ignore."""
    if has_param_groups(optim):
        raise ValueError(f"{who} does not support parameter groups (optim.groups / norm_weight_decay / "
                         f"bias_weight_decay); they work with sgd, adam and adamw on the native engine at "
                         f"zero.stage 0 and on the autograd engine")


def _group_patterns(g: Dict[str, Any], i: int) -> List[str]:
    if not isinstance(g, dict):
        raise ValueError(f"optim.groups[{i}]: expected a mapping with 'match', got {g!r}")
    bad = [k for k in g if k not in _GROUP_KEYS]
    if bad:
        raise KeyError(f"unknown config key {bad[0]!r} for optim.groups[{i}] (known: {', '.join(_GROUP_KEYS)})")
    m = g.get("match")
    pats = [m] if isinstance(m, str) else list(m or [])
    if not pats or not all(isinstance(x, str) for x in pats):
        raise ValueError(f"optim.groups[{i}]: 'match' must be a pattern or a list of patterns")
    return pats


def _group_value(v: Any, what: str) -> float:
    v = float(v)
    if not math.isfinite(v) or v < 0:
        raise ValueError(f"{what} must be finite and >= 0, got {v}")
    return v


def resolve_param_groups(named_kinds: Sequence[Tuple[str, str]], optim: Any) -> Optional[List[Tuple[float, float]]]:
    """Per-parameter ``(weight_decay, lr_mult)`` for ``[(name, kind)]`` (``kind``: weight | norm | bias; names
    as ``model.named_parameters()`` gives them), or None when ``optim`` sets no group field at all.

    ``optim.groups`` are tried in order against the name (``fnmatch`` patterns) and the first match wins;
    its ``weight_decay`` is absolute, its ``lr_mult`` multiplies the scheduled learning rate. A key the
    matching group leaves out (and every key of an unmatched parameter) falls through to
    ``norm_weight_decay`` (kind norm) / ``bias_weight_decay`` (kind bias) when >= 0, then to
    ``weight_decay`` and an ``lr_mult`` of 1."""
    if not has_param_groups(optim):
        return None
    base = float(optim.weight_decay)
    short = {}
    for kind, key in (("norm", "norm_weight_decay"), ("bias", "bias_weight_decay")):
        v = float(getattr(optim, key, -1.0))
        if math.isnan(v) or v == math.inf:
            raise ValueError(f"optim.{key} must be finite, got {v}")
        if v >= 0:
            short[kind] = v
    groups = []
    for i, g in enumerate(getattr(optim, "groups", None) or []):
        pats = _group_patterns(g, i)
        wd = _group_value(g["weight_decay"], f"optim.groups[{i}].weight_decay") if g.get("weight_decay") is not None else None
        lm = _group_value(g["lr_mult"], f"optim.groups[{i}].lr_mult") if g.get("lr_mult") is not None else None
        if not any(fnmatch.fnmatchcase(name, pat) for name, _ in named_kinds for pat in pats):
            raise ValueError(f"optim.groups[{i}] (match={g['match']!r}) matches no parameter")
        groups.append((pats, wd, lm))
    out = []
    for name, kind in named_kinds:
        if kind not in ("weight", "norm", "bias"):
            raise ValueError(f"parameter {name!r}: unknown kind {kind!r}")
        wd = lm = None
        for pats, gwd, glm in groups:
            if any(fnmatch.fnmatchcase(name, pat) for pat in pats):
                wd, lm = gwd, glm
                break
        if wd is None:
            wd = short.get(kind, base)
        out.append((float(wd), 1.0 if lm is None else float(lm)))
    return out


def distinct_param_groups(values: Sequence[Tuple[float, float]]) -> List[Tuple[float, float]]:
    """The distinct ``(weight_decay, lr_mult)`` pairs in first-seen order."""
    return list(dict.fromkeys(values))


# ----------------------------------------------------------------------------------------
_DUR = re.compile(r"^\s*(\d+(?:\.\d+)?)\s*(ep|ba|sp)\s*$")


def parse_duration(s: Union[str, int], steps_per_epoch: int, batch_size: int = 1) -> int:
    """Composer duration -> number of optimizer steps: ``"2ep"``, ``"100ba"``, ``"5000sp"`` (samples)."""
    if isinstance(s, int):
        return s * steps_per_epoch
    m = _DUR.match(s)
    if not m:
        raise ValueError(f"bad duration {s!r} (expected e.g. '2ep', '100ba', '5000sp')")
    v, unit = float(m.group(1)), m.group(2)
    if unit == "ep":
        return int(round(v * steps_per_epoch))
    if unit == "ba":
        return int(v)
    return int(v) // max(1, batch_size)


def _ds_auto(v: Any) -> bool:
    return isinstance(v, str) and v.strip().lower() == "auto"


def _ds_bool(v: Any, default: bool = False) -> bool:
    """DeepSpeed booleans: JSON true/false, or the strings "true"/"false" the reference writes
    (`deepspeed_config.py:19-21` has ``"enabled": "true"``); "auto" = ``default``."""
    if v is None or _ds_auto(v):
        return default
    if isinstance(v, str):
        s = v.strip().lower()
        if s in ("true", "1", "yes", "on"):
            return True
        if s in ("false", "0", "no", "off", ""):
            return False
        raise ValueError(f"not a DeepSpeed boolean: {v!r}")
    return bool(v)


def _ds_num(v: Any, auto: Union[int, float]) -> Union[int, float]:
    """A DeepSpeed number: int, float, numeric string ("5e8"), or "auto" -> ``auto``."""
    if _ds_auto(v):
        return auto
    return float(v) if isinstance(v, str) else v


# DeepSpeed's own optimizer defaults: a key the dict omits takes these, never a TrainConfig default.
# DeepSpeed builds "Adam" / "AdamW" as its FusedAdam (adam_w_mode for "AdamW"), whose weight_decay
# defaults to 0.0 -- not torch.optim.AdamW's 0.01 (the reference dicts omit the key,
# `02_deepspeed/deepspeed_config.py:22-32`, so their runs do not decay); SGD: torch's defaults.
#   "Lamb" is DeepSpeed's FusedLamb: weight decay 0.0, max_coeff 10.0, min_coeff 0.01 (its documented
# defaults; DeepSpeed is not installed where this was written, so they are taken from its documentation).
_DS_OPT_DEFAULTS = {"adamw": {"weight_decay": 0.0}, "adam": {"weight_decay": 0.0},
                    "sgd": {"weight_decay": 0.0, "momentum": 0.0},
                    "lamb": {"weight_decay": 0.0, "max_coeff": 10.0, "min_coeff": 0.01}}


def from_deepspeed(ds: Dict[str, Any], base: Optional[TrainConfig] = None, world_size: Optional[int] = None,
                   model_numel: Optional[int] = None) -> TrainConfig:
    """Map a DeepSpeed config dict (the schema `02_deepspeed/deepspeed_config.py:5-105` uses) onto a
    :class:`TrainConfig`. The reference dicts load verbatim:

    * ``"auto"`` values are resolved the way DeepSpeed's integration resolves them, with the model
      in place of a transformer's hidden size: ``train_batch_size`` = micro x accumulation x world,
      ``reduce_bucket_size`` / ``allgather_bucket_size`` = the whole gradient (``model_numel``; one
      bucket -- ResNet gradients are <= 102 MB), ``stage3_prefetch_bucket_size`` = 0.9 x that,
      ``stage3_param_persistence_threshold`` = DeepSpeed's default 1e5;
    * string booleans (``"true"`` / ``"false"``) are parsed, not truth-tested;
    * an explicit ``train_batch_size`` is checked against micro x accumulation x world (as DeepSpeed
      does) or, without a micro batch, defines it;
    * optimizer keys the dict omits take DeepSpeed's optimizer defaults (FusedAdam: weight decay 0.0
      for "Adam" and "AdamW"), not the TrainConfig's;
    * ``"Lamb"`` (DeepSpeed's FusedLamb) maps ``lr, betas, eps, weight_decay`` and ``max_coeff`` /
      ``min_coeff`` -> ``trust_max`` / ``trust_min``, with DeepSpeed's documented defaults (weight decay
      0.0, ``max_coeff`` 10.0, ``min_coeff`` 0.01), and sets ``adapt_1d`` (FusedLamb decays and adapts
      every tensor). DeepSpeed is not installed here: the defaults are its documentation's, unverified
      against its code;
    * WarmupLR keeps its ``warmup_type`` ("log" when absent, DeepSpeed's default).
    """
    cfg = copy.deepcopy(base) if base is not None else TrainConfig()
    if world_size is None:
        world_size = int(os.environ.get("WORLD_SIZE", "1"))
    ga = ds.get("gradient_accumulation_steps", 1)
    ga = 1 if _ds_auto(ga) else int(float(ga))
    cfg.grad_accum = ga
    mb = ds.get("train_micro_batch_size_per_gpu")
    if mb is not None and not _ds_auto(mb):
        cfg.batch_size = int(float(mb))
    tbs = ds.get("train_batch_size")
    if tbs is not None and not _ds_auto(tbs):
        tbs = int(float(tbs))
        if mb is None or _ds_auto(mb):
            if tbs % (ga * world_size):
                raise ValueError(f"train_batch_size {tbs} is not divisible by accumulation {ga} x world {world_size}")
            cfg.batch_size = tbs // (ga * world_size)
        elif tbs != cfg.batch_size * ga * world_size:
            raise ValueError(f"train_batch_size {tbs} != micro batch {cfg.batch_size} x accumulation {ga} x "
                             f"world {world_size}")
    if "gradient_clipping" in ds and not _ds_auto(ds["gradient_clipping"]):
        cfg.optim.grad_clip = float(ds["gradient_clipping"])
    if _ds_bool(ds.get("bf16", {}).get("enabled")) or _ds_bool(ds.get("fp16", {}).get("enabled")):
        cfg.precision = "bf16"  # fp16 dicts too: the MI355X path computes in bf16 (no loss scaling needed)
    elif "bf16" in ds or "fp16" in ds:
        cfg.precision = "fp32"
    if "steps_per_print" in ds:
        cfg.log_every = int(float(ds["steps_per_print"]))
    if "wall_clock_breakdown" in ds:
        cfg.wall_clock_breakdown = _ds_bool(ds["wall_clock_breakdown"])
    tb = ds.get("tensorboard") or {}
    if _ds_bool(tb.get("enabled")):
        cfg.tensorboard_dir = str(tb.get("output_path", ""))
    opt = ds.get("optimizer")
    if opt:
        t = opt.get("type", "AdamW").lower()
        if t not in ("adamw", "adam", "sgd", "lars", "lamb"):
            raise ValueError(f"unsupported DeepSpeed optimizer type {opt.get('type')!r}")
        cfg.optim.name = t
        p = dict(_DS_OPT_DEFAULTS.get(t, {}))
        p.update({"betas": (0.9, 0.999), "eps": 1e-8} if t in ("adamw", "adam", "lamb") else {})
        p.update({k: v for k, v in opt.get("params", {}).items() if not _ds_auto(v)})
        if "lr" in p:
            cfg.optim.lr = float(p["lr"])
        if "betas" in p:
            cfg.optim.betas = tuple(float(b) for b in p["betas"])
        if "eps" in p:
            cfg.optim.eps = float(p["eps"])
        if "weight_decay" in p:
            cfg.optim.weight_decay = float(p["weight_decay"])
        if "momentum" in p:
            cfg.optim.momentum = float(p["momentum"])
        if t == "lamb":  # FusedLamb clamps the trust ratio to [min_coeff, max_coeff] and adapts every tensor
            cfg.optim.trust_max = float(p["max_coeff"])
            cfg.optim.trust_min = float(p["min_coeff"])
            cfg.optim.adapt_1d = True
    sch = ds.get("scheduler")
    if sch:
        t = sch.get("type", "")
        p = {k: v for k, v in sch.get("params", {}).items() if not _ds_auto(v)}
        if t == "WarmupLR":
            cfg.sched.name = "warmup_lr"
            cfg.sched.warmup_steps = int(float(p.get("warmup_num_steps", 1000)))
            cfg.sched.warmup_min_lr = float(p.get("warmup_min_lr", 0.0))
            cfg.sched.warmup_type = str(p.get("warmup_type", "log"))
            if cfg.sched.warmup_type not in ("log", "linear"):
                raise ValueError(f"WarmupLR warmup_type must be 'log' or 'linear', got {cfg.sched.warmup_type!r}")
            if "warmup_max_lr" in p:
                cfg.optim.lr = float(p["warmup_max_lr"])
        elif t in ("WarmupDecayLR", "WarmupCosineLR"):
            cfg.sched.name = "warmup_linear" if t == "WarmupDecayLR" else "warmup_cosine"
            cfg.sched.warmup_steps = int(float(p.get("warmup_num_steps", 0)))
            cfg.sched.warmup_type = str(p.get("warmup_type", "log"))
            cfg.sched.total_steps = int(float(p.get("total_num_steps", 0)))
        elif t:
            raise ValueError(f"unsupported DeepSpeed scheduler type {t!r}")
    z = ds.get("zero_optimization")
    if z is not None:
        zc = cfg.zero
        zc.stage = int(float(z.get("stage", 0)))
        whole = int(model_numel) if model_numel else zc.reduce_bucket_size
        for k in ("reduce_bucket_size", "allgather_bucket_size", "sub_group_size", "stage3_max_live_parameters",
                  "stage3_max_reuse_distance"):
            if k in z:
                setattr(zc, k, int(_ds_num(z[k], whole if "bucket" in k else getattr(zc, k))))
        if "stage3_prefetch_bucket_size" in z:
            zc.stage3_prefetch_bucket_size = int(_ds_num(z["stage3_prefetch_bucket_size"], 0.9 * whole))
        if "stage3_param_persistence_threshold" in z:
            zc.stage3_param_persistence_threshold = int(_ds_num(z["stage3_param_persistence_threshold"], 100_000))
        for k in ("overlap_comm", "contiguous_gradients", "reduce_scatter", "allgather_partitions",
                  "stage3_gather_16bit_weights_on_model_save"):
            if k in z:
                setattr(zc, k, _ds_bool(z[k], getattr(zc, k)))

        def _dev(key):
            d = z.get(key) or {}
            return str(d.get("device", "none")).lower() not in ("none", "") if isinstance(d, dict) else _ds_bool(d)
        zc.offload_optimizer = _dev("offload_optimizer") or _ds_bool(z.get("cpu_offload"))
        zc.offload_param = _dev("offload_param")
    cfg.deepspeed_applied = True  # train() then skips the launcher's DBX_DEEPSPEED_CONFIG env copy
    return cfg
