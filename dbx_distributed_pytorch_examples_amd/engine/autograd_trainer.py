"""Generic training step for any ``nn.Module`` (models the native ResNet program does not cover:
the MNIST ``Net``, frozen-backbone heads, Composer-style models, user modules) and for CPU hosts.

Stock autograd + our flat-bucket DDP (``parallel.ddp``) + bf16 autocast on the GPU
(channels_last memory format), torch optimizers (or the flat ZeRO optimizer). Loss: the model's
own ``loss(outputs, batch)`` if it has one (Composer convention), NLL for log-probability outputs
(the reference MNIST ``Net`` ends in ``log_softmax``, `01_basic_torch_distributor.py:91,99`), else
cross-entropy with optional label smoothing; optional CutMix on the batch (Composer algorithm).
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..config import distinct_param_groups, has_param_groups, resolve_param_groups, validate_loss
from ..parallel.ddp import DistributedDataParallel, flat_view, unwrap


def _single_group(params, who: str):
    """LARS and LAMB decide decay and adaptation per tensor themselves: no torch param groups."""
    params = list(params)
    if params and isinstance(params[0], dict):
        raise ValueError(f"{who} has its own per-tensor decay / adapt rule and takes no parameter groups")
    return params


class LARS(torch.optim.Optimizer):
    """SGD-momentum with layer-wise adaptive rate scaling (You et al., large-batch ImageNet): for every
    tensor with ndim > 1, g <- eta*|w|/(|g| + wd*|w|) * (g + wd*w); 1-d tensors (BN, biases) take the
    plain gradient without decay. Same math as the native ``lars_scale`` + ``sgd_step`` kernels."""

    def __init__(self, params, lr, momentum=0.9, weight_decay=0.0, trust_coefficient=0.001, nesterov=False):
        params = _single_group(params, "LARS")
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay, eta=trust_coefficient,
                                      nesterov=nesterov))

    @torch.no_grad()
    def step(self, closure=None):
        for grp in self.param_groups:
            for p in grp["params"]:
                if p.grad is None:
                    continue
                d = p.grad
                if p.ndim > 1:
                    wn, gn = p.norm(), d.norm()
                    trust = torch.where((wn > 0) & (gn > 0), grp["eta"] * wn / (gn + grp["weight_decay"] * wn),
                                        torch.ones_like(wn))
                    d = (d + grp["weight_decay"] * p) * trust
                st = self.state[p]
                if grp["momentum"]:
                    buf = st.get("momentum_buffer")
                    if buf is None:
                        buf = st["momentum_buffer"] = d.clone()
                    else:
                        buf.mul_(grp["momentum"]).add_(d)
                    d = d + grp["momentum"] * buf if grp["nesterov"] else buf
                p.add_(d, alpha=-grp["lr"])


class LAMB(torch.optim.Optimizer):
    """LAMB (You et al., layer-wise adaptive moments): Adam moments with bias correction, r = mhat /
    (sqrt(vhat) + eps); tensors with ndim > 1 (every tensor with ``adapt_1d``) take u = r + wd*w and the
    trust ratio t = |w|/|u| (1 when either norm is 0), clamped to [trust_min, trust_max] (a bound of 0 is
    no bound); the others take u = r, t = 1; w -= lr*t*u. Same math as the native ``lamb_step`` kernels."""

    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, adapt_1d=False, trust_min=0.0,
                 trust_max=0.0):
        params = _single_group(params, "LAMB")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay,
                                      adapt_1d=bool(adapt_1d), trust_min=trust_min, trust_max=trust_max))

    @torch.no_grad()
    def step(self, closure=None):
        for grp in self.param_groups:
            b1, b2 = grp["betas"]
            for p in grp["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["exp_avg"], st["exp_avg_sq"] = torch.zeros_like(p), torch.zeros_like(p)
                st["step"] += 1
                m, v, g = st["exp_avg"], st["exp_avg_sq"], p.grad
                m.mul_(b1).add_(g, alpha=1 - b1)
                v.mul_(b2).addcmul_(g, g, value=1 - b2)
                u = (m / (1 - b1 ** st["step"])) / (torch.sqrt(v / (1 - b2 ** st["step"])) + grp["eps"])
                if p.ndim > 1 or grp["adapt_1d"]:
                    u = u + grp["weight_decay"] * p
                    wn, un = p.norm(), u.norm()
                    t = torch.where((wn > 0) & (un > 0), wn / un, torch.ones_like(wn))
                    if grp["trust_min"] > 0:
                        t = t.clamp(min=grp["trust_min"])
                    if grp["trust_max"] > 0:
                        t = t.clamp(max=grp["trust_max"])
                    u = u * t
                p.add_(u, alpha=-grp["lr"])


def param_kinds(model: nn.Module) -> dict:
    """``{parameter name: kind}`` for config.resolve_param_groups: "norm" for the direct parameters of a
    normalisation layer, "bias" for any other parameter named ``bias``, else "weight"."""
    norm = (nn.modules.batchnorm._NormBase, nn.GroupNorm, nn.LayerNorm)
    norm_ids = {id(p) for m in model.modules() if isinstance(m, norm) for p in m.parameters(recurse=False)}
    return {n: "norm" if id(p) in norm_ids else "bias" if n.split(".")[-1] == "bias" else "weight"
            for n, p in model.named_parameters()}


def build_torch_optimizer(params, o, model: Optional[nn.Module] = None):
    """``params``: parameters, or ``(name, parameter)`` pairs as ``model.named_parameters()`` gives them.
    With parameter groups in ``o`` (config.resolve_param_groups; needs the pairs and ``model`` for the
    kinds) one torch param group per distinct (weight_decay, lr_mult): ``lr = o.lr * lr_mult`` and an
    ``lr_mult`` entry that ``AutogradTrainer.set_lr`` keeps applying."""
    params = list(params)
    named = bool(params) and isinstance(params[0], tuple)
    if has_param_groups(o):
        if o.name in ("lars", "lamb"):
            raise ValueError(f"{o.name.upper()} has its own per-tensor decay / adapt rule and takes no parameter groups")
        if not named or model is None:
            raise ValueError("parameter groups need named parameters and the model (for the parameter kinds)")
        kinds = param_kinds(model)
        values = resolve_param_groups([(n, kinds.get(n, "weight")) for n, _ in params], o)
        params = [{"params": [p for (_, p), v in zip(params, values) if v == (wd, lm)], "weight_decay": wd,
                   "lr": o.lr * lm, "lr_mult": lm} for wd, lm in distinct_param_groups(values)]
    elif named:
        params = [p for _, p in params]
    if o.name == "lamb":
        return LAMB(params, lr=o.lr, betas=tuple(o.betas), eps=o.eps, weight_decay=o.weight_decay,
                    adapt_1d=getattr(o, "adapt_1d", False), trust_min=getattr(o, "trust_min", 0.0),
                    trust_max=getattr(o, "trust_max", 0.0))
    if o.name == "lars":
        return LARS(params, lr=o.lr, momentum=o.momentum, weight_decay=o.weight_decay,
                    trust_coefficient=getattr(o, "trust_coefficient", 0.001), nesterov=o.nesterov)
    if o.name == "sgd":
        return torch.optim.SGD(params, lr=o.lr, momentum=o.momentum, dampening=getattr(o, "dampening", 0.0),
                               nesterov=o.nesterov, weight_decay=o.weight_decay)
    if o.name == "adam":
        return torch.optim.Adam(params, lr=o.lr, betas=tuple(o.betas), eps=o.eps, weight_decay=o.weight_decay)
    if o.name == "adamw":
        return torch.optim.AdamW(params, lr=o.lr, betas=tuple(o.betas), eps=o.eps, weight_decay=o.weight_decay)
    raise ValueError(f"unknown optimizer {o.name!r}")


def cutmix(x: torch.Tensor, y: torch.Tensor, num_classes: int, alpha: float, gen: Optional[torch.Generator] = None):
    """CutMix (Composer ``CutMix(alpha)``, `03_composer/01_cifar_composer_resnet.ipynb:430`): paste a
    box from a permuted batch, mix one-hot targets by the pasted area."""
    lam = torch.distributions.Beta(alpha, alpha).sample().item() if alpha > 0 else 1.0
    B, _, H, W = x.shape
    perm = torch.randperm(B, device=x.device)
    rh, rw = int(H * math.sqrt(1 - lam)), int(W * math.sqrt(1 - lam))
    cy, cx = torch.randint(0, H, (1,)).item(), torch.randint(0, W, (1,)).item()
    y0, y1 = max(cy - rh // 2, 0), min(cy + rh // 2, H)
    x0, x1 = max(cx - rw // 2, 0), min(cx + rw // 2, W)
    x = x.clone()
    x[:, :, y0:y1, x0:x1] = x[perm, :, y0:y1, x0:x1]
    lam = 1 - (y1 - y0) * (x1 - x0) / (H * W)
    t = F.one_hot(y, num_classes).float()
    return x, lam * t + (1 - lam) * t[perm]


def _beta(alpha: float, gen: Optional[torch.Generator] = None) -> float:
    """One Beta(alpha, alpha) draw (two gamma draws when a generator is given)."""
    if gen is None:
        return torch.distributions.Beta(alpha, alpha).sample().item()
    g = torch._standard_gamma(torch.full((2,), float(alpha), device=gen.device), generator=gen)
    return (g[0] / g.sum().clamp_min(1e-30)).item()


def mixup(x: torch.Tensor, y: torch.Tensor, num_classes: int, alpha: float, gen: Optional[torch.Generator] = None):
    """MixUp (torchvision's ResNet-50 recipe: alpha 0.2): ``lam ~ Beta(alpha, alpha)``, every sample blended
    with one of a permuted batch, ``lam x + (1 - lam) x[perm]``, one-hot targets mixed by the same weight --
    the native step's semantics (K.augment_u8 ``blend``) on the float batch."""
    lam = _beta(alpha, gen) if alpha > 0 else 1.0
    perm = torch.randperm(x.shape[0], generator=gen, device=gen.device if gen is not None else "cpu").to(x.device)
    t = F.one_hot(y, num_classes).float()
    return lam * x + (1 - lam) * x[perm], lam * t + (1 - lam) * t[perm]


def random_erase(x: torch.Tensor, p: float, scale=(0.02, 1 / 3), ratio=(0.3, 3.3), mode: str = "const",
                 gen: Optional[torch.Generator] = None) -> torch.Tensor:
    """Random erasing of a normalised float batch [B, C, H, W], torchvision's rule per sample: with
    probability ``p`` up to 10 tries of ``area = H W U(scale)`` and a log-uniform aspect ratio; the first
    with ``1 <= h < H`` and ``1 <= w < W`` is erased at a uniform position -- to 0 (``"const"``) or to N(0, 1)
    noise per pixel and channel (``"pixel"``); a sample none of whose tries fits stays as it is. Applied
    before any mixing, so the rectangle travels with its sample (the native step's semantics)."""
    if mode not in ("const", "pixel"):
        raise ValueError(f'mode must be "const" or "pixel", got {mode!r}')
    B, C, H, W = x.shape
    dev = gen.device if gen is not None else torch.device("cpu")
    chosen = (torch.rand(B, generator=gen, device=dev) < p).nonzero().flatten().tolist()
    if not chosen:
        return x
    x = x.clone()
    l0, l1 = math.log(ratio[0]), math.log(ratio[1])
    for i in chosen:
        for _ in range(10):
            u = torch.rand(2, generator=gen, device=dev).tolist()
            area, ar = H * W * (scale[0] + (scale[1] - scale[0]) * u[0]), math.exp(l0 + (l1 - l0) * u[1])
            h, w = int(round(math.sqrt(area * ar))), int(round(math.sqrt(area / ar)))
            if not (1 <= h < H and 1 <= w < W):
                continue
            v = torch.rand(2, generator=gen, device=dev).tolist()
            y0, x0 = min(int(v[0] * (H - h + 1)), H - h), min(int(v[1] * (W - w + 1)), W - w)
            x[i, :, y0:y0 + h, x0:x0 + w] = 0.0 if mode == "const" else \
                torch.randn(C, h, w, generator=gen, device=dev).to(x)
            break
    return x


def soft_cross_entropy(logits: torch.Tensor, target: torch.Tensor, smoothing: float = 0.0) -> torch.Tensor:
    if smoothing:
        target = target * (1 - smoothing) + smoothing / target.shape[1]
    return -(target * F.log_softmax(logits.float(), 1)).sum(1).mean()


def bce_loss(logits: torch.Tensor, labels: Optional[torch.Tensor], smoothing: float = 0.0,
             target_threshold: Optional[float] = None, sum_classes: bool = False,
             target: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The autograd engines' binary cross-entropy: ``F.binary_cross_entropy_with_logits`` on the targets of
    ``reference.bce_logits`` (its definition) -- from ``labels``, or from mixed one-hot rows ``target``."""
    from ..ops import reference as R
    logits = logits.float()
    if target is not None:
        t = R.bce_soft_targets(target.float(), smoothing, target_threshold)
    else:
        t = R.bce_targets(labels, logits.shape[1], smoothing, target_threshold=target_threshold)
    return R.bce_with_logits_loss(logits, t, sum_classes)


class AutogradTrainer:
    def __init__(self, model: nn.Module, device: torch.device, optim, label_smoothing: float = 0.0,
                 bucket_cap_mb: float = 64.0, channels_last: bool = True, zero_stage: int = 0,
                 cutmix_alpha: float = 0.0, grad_accum: int = 1, allreduce_dtype=torch.float32,
                 offload_optimizer: bool = False, offload_param: bool = False, bf16: bool = True,
                 stage3: Optional[dict] = None, mixup_alpha: float = 0.0, mix_prob: float = 1.0,
                 mix_switch_prob: float = 0.5, erase_prob: float = 0.0, erase_mode: str = "const",
                 erase_scale=(0.02, 1 / 3), erase_ratio=(0.3, 3.3), auto_augment=None, loss: str = "ce",
                 bce_target_threshold: Optional[float] = None, bce_sum_classes: bool = False,
                 drop_path_rate: float = 0.0, src_ragged=None):
        from ..config import validate_drop_path
        if src_ragged is not None:  # refused, never ignored
            raise ValueError(f"src_ragged={src_ragged!r} needs the native training step (NativeTrainer), whose input "
                             f"kernels crop every image from its own size; the autograd engine takes dense batches")
        if validate_drop_path(drop_path_rate) != 0.0:  # refused, never ignored
            raise ValueError(f"drop_path_rate={drop_path_rate!r} is built into the native training step (NativeTrainer: "
                             f"gates on the blocks' last BatchNorm); the autograd engine runs the module as it is -- "
                             f"put torchvision.ops.StochasticDepth into the model instead")
        if auto_augment is not None:  # refused, never ignored
            raise ValueError(f"auto_augment={auto_augment!r} runs in the native step's input kernels (NativeTrainer); "
                             f"the autograd engine has no such stage -- put data.transforms.TrivialAugmentWide in the "
                             f"dataset's transform chain instead")
        from .mix import validate_mix
        validate_mix(mixup_alpha, cutmix_alpha, mix_prob, mix_switch_prob, erase_prob, erase_mode, erase_scale,
                     erase_ratio)
        validate_loss(loss, bce_target_threshold, bce_sum_classes)
        m = unwrap(model)
        if loss == "bce" and (callable(getattr(m, "loss", None)) or getattr(m, "outputs_log_probs", False)
                              or isinstance(m, _log_prob_types())):  # refused, never ignored
            raise ValueError(f"loss='bce' needs a model that returns logits and leaves the loss to the trainer; "
                             f"{type(m).__name__} brings its own loss or returns log-probabilities")
        self.loss, self.bce_target_threshold, self.bce_sum_classes = loss, bce_target_threshold, bool(bce_sum_classes)
        self.dev = device
        self.bf16 = bool(bf16) and device.type == "cuda"  # autocast bf16 (DeepSpeed bf16.enabled)
        self.model = model.to(device)
        if device.type == "cuda" and channels_last:
            self.model = self.model.to(memory_format=torch.channels_last)
        self.sharded = zero_stage == 3 or offload_optimizer or offload_param
        if self.sharded:  # ZeRO-3: parameters, gradients and optimizer state sharded (parallel/fsdp.py)
            from ..parallel.fsdp import ShardedDataParallel
            self.ddp = ShardedDataParallel(self.model, optim, offload_optimizer=offload_optimizer,
                                           offload_param=offload_param, **(stage3 or {}))
            zero_stage = 0
        else:
            from .native_module import NativeResNet
            # a native_module inside averages its own gradients (overlapped, per backward segment)
            own_sync = any(isinstance(m, NativeResNet) for m in self.model.modules())
            self.ddp = DistributedDataParallel(self.model, bucket_cap_mb=bucket_cap_mb, allreduce_dtype=allreduce_dtype,
                                               gradient_sync=not own_sync)
        self.world = self.ddp.world
        self.o = optim
        self.smoothing = label_smoothing
        self.cutmix_alpha = cutmix_alpha
        # MixUp, the per-step choice between it and CutMix, random erasing: the native step's rules (engine/mix.py)
        self.mixup_alpha, self.mix_prob, self.mix_switch_prob = mixup_alpha, mix_prob, mix_switch_prob
        self.erase_prob, self.erase_mode = erase_prob, erase_mode
        self.erase_scale, self.erase_ratio = tuple(erase_scale), tuple(erase_ratio)
        self.grad_accum = max(1, grad_accum)
        self.num_classes = getattr(unwrap(model), "num_classes", None)
        self.zero = None
        named = [(n, p) for n, p in self.model.named_parameters() if p.requires_grad]
        params = [p for _, p in named]
        if self.sharded:
            self.opt = None
        elif zero_stage and params:
            from ..parallel.zero import ZeroShardedOptimizer
            # ZeRO over the DDP flat gradient buffer: master = flat copy of params in the same order
            self._zero_master = torch.zeros_like(self.ddp.flat.buffer)
            for p, off in zip(self.ddp._params, self.ddp.flat.offsets):
                flat_view(self._zero_master, off, p).copy_(p.detach())  # the gradients' memory order
            self.zero = ZeroShardedOptimizer(self._zero_master, self.ddp.flat.buffer, optim, stage=zero_stage,
                                             grad_scale=1.0)  # DDP already averaged
            self.opt = None
        else:
            self.opt = build_torch_optimizer(named, optim, self.model) if params else None
        self.micro = 0
        self.loss_sum = torch.zeros((), device=device)
        self.correct = torch.zeros((), device=device)
        self.count = 0

    def set_lr(self, lr: float):
        self.o.lr = lr
        if self.opt is not None:
            for g in self.opt.param_groups:
                g["lr"] = lr * g.get("lr_mult", 1.0)

    def _mix_kind(self) -> str:
        """This step's mixing: none with probability 1 - mix_prob, else CutMix with probability
        mix_switch_prob when both alphas are set (never both in one step)."""
        cut, mix = self.cutmix_alpha > 0, self.mixup_alpha > 0
        if not (cut or mix):
            return "none"
        if self.mix_prob < 1.0 and not torch.rand(()).item() < self.mix_prob:
            return "none"
        if cut and mix:
            return "cutmix" if torch.rand(()).item() < self.mix_switch_prob else "mixup"
        return "cutmix" if cut else "mixup"

    def _loss(self, out, x, y, target=None):
        m = unwrap(self.model)
        if self.loss == "bce":
            return bce_loss(out, y, self.smoothing, self.bce_target_threshold, self.bce_sum_classes, target=target)
        if hasattr(m, "loss") and callable(m.loss) and target is None:
            return m.loss(out, (x, y), label_smoothing=self.smoothing) if "label_smoothing" in m.loss.__code__.co_varnames \
                else m.loss(out, (x, y))
        if target is not None:
            return soft_cross_entropy(out, target, self.smoothing)
        if getattr(m, "outputs_log_probs", False) or isinstance(m, _log_prob_types()):
            return F.nll_loss(out.float(), y)
        return F.cross_entropy(out.float(), y, label_smoothing=self.smoothing)

    def step(self, x: torch.Tensor, y: torch.Tensor) -> None:
        self.model.train()
        x = x.to(self.dev, non_blocking=True)
        y = y.to(self.dev, non_blocking=True)
        if self.dev.type == "cuda" and x.dim() == 4:
            x = x.contiguous(memory_format=torch.channels_last)
        target = None
        if self.erase_prob > 0 and x.dim() == 4:  # per sample, before any mixing
            x = random_erase(x, self.erase_prob, self.erase_scale, self.erase_ratio, self.erase_mode)
        kind = self._mix_kind() if self.num_classes else "none"
        if kind == "cutmix":
            x, target = cutmix(x, y, self.num_classes, self.cutmix_alpha)
        elif kind == "mixup":
            x, target = mixup(x, y, self.num_classes, self.mixup_alpha)
        last_micro = (self.micro + 1) % self.grad_accum == 0
        ctx = self.ddp.no_sync() if not last_micro else _null()
        with ctx:
            with torch.autocast(self.dev.type, dtype=torch.bfloat16, enabled=self.bf16):
                out = self.ddp(x) if not _is_composer(self.model) else self.ddp((x, y))
            loss = self._loss(out, x, y, target) / self.grad_accum
            loss.backward()
        self.loss_sum += loss.detach().float() * self.grad_accum * y.shape[0]
        self.correct += (out.detach().argmax(1) == y).sum()
        self.count += y.shape[0]
        self.micro += 1
        if not last_micro:
            return
        self.ddp.finish_gradient_sync()
        if self.sharded:
            self.ddp.optimizer_step()
            self.ddp.zero_grad()
            return
        if self.o.grad_clip and self.zero is None:
            torch.nn.utils.clip_grad_norm_([p for p in self.model.parameters() if p.grad is not None], self.o.grad_clip)
        if self.zero is not None:
            self.zero.step(grads_already_reduced=True)
            with torch.no_grad():
                for p, off in zip(self.ddp._params, self.ddp.flat.offsets):
                    p.copy_(flat_view(self._zero_master, off, p))
        elif self.opt is not None:
            self.opt.step()
        self.ddp.zero_grad()

    def read_metrics(self, reset: bool = True) -> Tuple[float, float]:
        if self.sharded:  # epoch end (all ranks): full parameters for evaluation / rank-0 checkpoints
            self.ddp.gather_full_params()
        loss, corr = float(self.loss_sum.item()), float(self.correct.item())
        if reset:
            self.loss_sum.zero_()
            self.correct.zero_()
            self.count = 0
        return loss, corr

    def _eval_logits(self, x, y):
        self.model.eval()
        x, y = x.to(self.dev), y.to(self.dev)
        if self.dev.type == "cuda" and x.dim() == 4:
            x = x.contiguous(memory_format=torch.channels_last)
        with torch.autocast(self.dev.type, dtype=torch.bfloat16, enabled=self.bf16):
            out = self.model((x, y)) if _is_composer(self.model) else self.model(x)
        return out.float(), y

    @torch.no_grad()
    def eval_stats(self, x, y, stats: torch.Tensor, topk: int = 5) -> None:
        """Add the batch's [loss sum, top-1, top-k, count] to ``stats`` (fp64 [4] on the trainer's device)
        by ``reference.ce_eval``: no host sync. ``topk`` is clipped to the class count (0 counts top-1).
        A model that returns log-probabilities gets ``lse(x) - x_l = -x_l`` up to fp32 rounding."""
        from ..ops import reference as R
        out, y = self._eval_logits(x, y)
        out = out.reshape(out.shape[0], -1).contiguous()
        R.ce_eval(out, y.long(), stats, max(1, min(int(topk), out.shape[1])))

    @torch.no_grad()
    def eval_batch(self, x, y) -> Tuple[float, int]:
        out, y = self._eval_logits(x, y)
        m = unwrap(self.model)
        if isinstance(m, _log_prob_types()):
            loss = F.nll_loss(out, y, reduction="sum")
        else:
            loss = F.cross_entropy(out, y, reduction="sum")
        return float(loss.item()), int((out.argmax(1) == y).sum().item())


def _log_prob_types():
    from ..models.mnist import Net
    return (Net,)


def _is_composer(model) -> bool:
    from ..models.wrappers import ComposerResNet50
    return isinstance(unwrap(model), ComposerResNet50)


class _null:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False
