"""The binary cross-entropy training loss outside the kernel: the three config fields, their validation and
``loss_options``, the new config file, the autograd engine's loss against the float64 definition, the refusals,
the native trainer's wiring on the CPU reference path, and ``train()`` end to end on the CPU."""
import copy
import math
import os

import pytest
import torch
import torch.nn as nn

from dbx_distributed_pytorch_examples_amd import config as C
from dbx_distributed_pytorch_examples_amd.ops import kernels as K

CPU = torch.device("cpu")
ROOT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs")


def test_fields_round_trip(tmp_path):
    d = C.TrainConfig().data
    assert (d.loss, d.bce_target_threshold, d.bce_sum_classes) == ("ce", None, False)
    assert C.loss_options(d) == dict(loss="ce", bce_target_threshold=None, bce_sum_classes=False)
    cfg = C.load_config(overrides=["data.loss=bce", "data.bce_target_threshold=0.2", "data.bce_sum_classes=true"])
    assert C.loss_options(cfg.data) == dict(loss="bce", bce_target_threshold=0.2, bce_sum_classes=True)
    path = tmp_path / "c.yaml"
    path.write_text("model: resnet18\ndata: {loss: bce, bce_target_threshold: 0.25, bce_sum_classes: true}\n")
    cfg = C.load_config(str(path))
    assert C.loss_options(cfg.data) == dict(loss="bce", bce_target_threshold=0.25, bce_sum_classes=True)
    again = C.load_config(str(path), overrides=["data.bce_target_threshold=0.5", "data.bce_sum_classes=false"])
    assert C.loss_options(again.data) == dict(loss="bce", bce_target_threshold=0.5, bce_sum_classes=False)
    assert C.to_dict(cfg)["data"]["loss"] == "bce"


@pytest.mark.parametrize("kw", [dict(loss="focal"), dict(loss=None), dict(loss="ce", bce_target_threshold=0.2),
                                dict(loss="ce", bce_sum_classes=True), dict(loss="bce", bce_target_threshold=1.0),
                                dict(loss="bce", bce_target_threshold=-0.1), dict(loss="bce", bce_target_threshold="0.2"),
                                dict(loss="bce", bce_target_threshold=float("nan")), dict(loss="bce", bce_sum_classes=1)])
def test_validate_data_refuses(kw):
    d = C.TrainConfig().data
    for k, v in kw.items():
        setattr(d, k, v)
    with pytest.raises(ValueError):
        C.validate_data(d)
    with pytest.raises(ValueError):
        C.loss_options(d)


def test_validate_data_accepts():
    d = C.TrainConfig().data
    for thr, sc in ((None, False), (0.0, True), (0.2, False), (0.999, True)):
        d.loss, d.bce_target_threshold, d.bce_sum_classes = "bce", thr, sc
        C.validate_data(d)


def test_the_config_file_is_the_lamb_config_plus_the_loss():
    bce = C.load_config(os.path.join(ROOT, "resnet50_imagenet_8192_lamb_bce.yaml"))
    base = C.load_config(os.path.join(ROOT, "resnet50_imagenet_8192_lamb.yaml"))
    C.validate_data(bce.data)
    assert C.loss_options(bce.data) == dict(loss="bce", bce_target_threshold=0.2, bce_sum_classes=False)
    assert (bce.data.label_smoothing, bce.data.mixup_alpha, bce.data.cutmix_alpha, bce.ema_decay) == (0.0, 0.1, 1.0, 0.0)
    assert base.data.loss == "ce" and base.ema_decay == 0.0
    for k, v in (("loss", "ce"), ("bce_target_threshold", None), ("label_smoothing", 0.1), ("mixup_alpha", 0.0),
                 ("cutmix_alpha", 0.0)):
        setattr(bce.data, k, v)
    assert C.to_dict(bce) == C.to_dict(base)
    head = open(os.path.join(ROOT, "resnet50_imagenet_8192_lamb_bce.yaml")).read().split("model:")[0]
    for words in ("in the spirit of", "UNTUNED", "repeated augmentation", "RandAugment", "stochastic depth"):
        assert words in head, words


# ---------------------------------------------------------------------------------------------
class Tiny(nn.Module):
    num_classes = 5

    def __init__(self):
        super().__init__()
        self.fc = nn.Linear(3 * 4 * 4, 5)

    def forward(self, x):
        return self.fc(x.flatten(1))


def definition64(model, x, t, sum_classes):
    """float64: the scalar loss of the definition for targets ``t`` [B, C], and d loss / d parameters."""
    m = copy.deepcopy(model).double()
    out = m(x.double())
    l = out.clamp(min=0) - out * t + torch.log1p(torch.exp(-out.abs()))
    loss = l.sum(1).mean() if sum_classes else l.mean()
    loss.backward()
    return float(loss.detach()), [p.grad.clone() for p in m.parameters()]


def targets64(y, y2, lam, C_, s, thr):
    idx = torch.arange(C_)[None, :]
    t = (1 - s) * ((idx == y[:, None]).double() * lam + (idx == y2[:, None]).double() * (1 - lam)) + s / C_
    return (t > thr).double() if thr is not None else t


@pytest.mark.parametrize("mixed", [False, True], ids=["labels", "mixed"])
@pytest.mark.parametrize("sum_classes", [False, True], ids=["mean", "sum"])
@pytest.mark.parametrize("s,thr", [(0.0, None), (0.1, 0.2)])
def test_autograd_trainer_loss_and_grad(s, thr, sum_classes, mixed):
    from dbx_distributed_pytorch_examples_amd.engine import autograd_trainer as A
    torch.manual_seed(0)
    model = Tiny()
    ref = copy.deepcopy(model)
    B = 6
    x = torch.randn(B, 3, 4, 4)
    y = torch.randint(0, 5, (B,))
    # two micro-steps per update: after the first, .grad holds d(loss / 2) and nothing has been zeroed
    tr = A.AutogradTrainer(model, CPU, C.OptimizerConfig(name="sgd", lr=0.1), label_smoothing=s, grad_accum=2,
                           loss="bce", bce_target_threshold=thr, bce_sum_classes=sum_classes,
                           mixup_alpha=0.4 if mixed else 0.0)
    if mixed:  # the step's own draw, replayed from the same seed
        torch.manual_seed(11)
        xm, target = A.mixup(x.clone(), y, 5, 0.4)
        t = (1 - s) * target.double() + s / 5
        t = (t > thr).double() if thr is not None else t
        assert bool(((target > 0).sum(1) >= 1).all()) and bool((target.sum(1) - 1).abs().max() < 1e-6)
        torch.manual_seed(11)
    else:
        xm, t = x, targets64(y, y, 1.0, 5, s, thr)
    tr.step(x.clone(), y)
    want, grads = definition64(ref, xm, t, sum_classes)
    got = float(tr.loss_sum) / B
    assert math.isclose(got, want, rel_tol=1e-5), (got, want)
    for p, g in zip(model.parameters(), grads):
        assert torch.allclose(p.grad.double() * 2, g, rtol=1e-4, atol=1e-6)


def test_refused_never_ignored():
    from dbx_distributed_pytorch_examples_amd.engine.autograd_trainer import AutogradTrainer
    from dbx_distributed_pytorch_examples_amd.engine.frozen_trainer import FrozenFeatureTrainer
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer
    from dbx_distributed_pytorch_examples_amd.models import FrozenBackboneClassifier, build_model
    from dbx_distributed_pytorch_examples_amd.models.mnist import Net
    from dbx_distributed_pytorch_examples_amd.models.wrappers import ComposerResNet50
    o = C.OptimizerConfig()
    with pytest.raises(ValueError, match="own loss"):
        AutogradTrainer(ComposerResNet50(num_classes=10), CPU, o, loss="bce")
    with pytest.raises(ValueError, match="log-probabilities"):
        AutogradTrainer(Net(), CPU, o, loss="bce")
    for bad in (dict(loss="focal"), dict(bce_target_threshold=0.2), dict(loss="ce", bce_sum_classes=True)):
        with pytest.raises(ValueError):
            AutogradTrainer(Tiny(), CPU, o, **bad)
        with pytest.raises(ValueError):
            NativeTrainer(build_model("resnet18", num_classes=10), 4, (32, 32), CPU, **bad)
        with pytest.raises(ValueError):
            FrozenFeatureTrainer(FrozenBackboneClassifier("resnet18", num_classes=10), 4, (32, 32), CPU, o, **bad)
    AutogradTrainer(ComposerResNet50(num_classes=10), CPU, o)  # its own loss stays available under "ce"


def test_native_trainer_wiring_on_the_reference_path():
    """CPU tensors run ops/reference.py: the step's dlogits and metrics are K.bce_logits of its logits, a
    softmax-CE trainer's are not, and an evaluation forward stays softmax CE."""
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig
    from dbx_distributed_pytorch_examples_amd.models import build_model
    torch.manual_seed(0)
    m1 = build_model("resnet18", num_classes=10)
    m2 = copy.deepcopy(m1)
    g = torch.Generator().manual_seed(1)
    img = torch.randint(0, 256, (4, 32, 32, 3), dtype=torch.uint8, generator=g)
    lab = torch.randint(0, 10, (4,), generator=g)
    tr = NativeTrainer(m1, 4, (32, 32), CPU, optim=OptimConfig(lr=0.05), use_graphs=False, label_smoothing=0.1,
                       loss="bce", bce_target_threshold=0.2, bce_sum_classes=True)
    ce = NativeTrainer(m2, 4, (32, 32), CPU, optim=OptimConfig(lr=0.05), use_graphs=False, label_smoothing=0.1)
    tr.step(img, lab)
    ce.step(img, lab)
    p = tr.prog
    assert torch.equal(p.logits, ce.prog.logits) and not torch.equal(p.dlogits, ce.prog.dlogits)
    dl, st = torch.empty_like(p.dlogits), torch.zeros(2, dtype=torch.float64)
    K.bce_logits(p.logits.clone(), lab, dl, None, st, smoothing=0.1, target_threshold=0.2, sum_classes=True)
    assert torch.equal(p.dlogits, dl) and torch.equal(p.metrics, st)
    assert tr.loss_summary() == dict(loss="bce", label_smoothing=0.1, bce_target_threshold=0.2, bce_sum_classes=True,
                                     kernel="bce_logits")
    assert ce.loss_summary()["kernel"] == "softmax_ce"
    assert not torch.equal(tr.prog.master, ce.prog.master)


def test_train_runs_on_the_cpu(monkeypatch):
    from dbx_distributed_pytorch_examples_amd.data.datasets import SyntheticImages
    from dbx_distributed_pytorch_examples_amd.train import engine as E
    monkeypatch.setenv("DBX_FORCE_CPU", "1")
    cfg = C.TrainConfig(model="tiny", num_classes=5, batch_size=4, epochs=1, max_steps=3, log_every=0, engine="autograd")
    cfg.optim.lr = 0.01
    cfg.data.num_workers = 0
    cfg.data.loss, cfg.data.bce_target_threshold, cfg.data.mixup_alpha = "bce", 0.2, 0.2
    seen = {}
    real = E._Autograd

    def spy(*a, **kw):
        r = real(*a, **kw)
        seen["tr"] = r.tr
        return r
    monkeypatch.setattr(E, "_Autograd", spy)
    torch.manual_seed(0)

    def to_tensor(img):
        import numpy as np
        return torch.from_numpy(np.array(img)).permute(2, 0, 1).float() / 255
    res = E.train(cfg, model=Tiny4(), train_dataset=SyntheticImages(12, 4, 3, 5, seed=1, transform=to_tensor),
                  log_mlflow=False)
    assert res.engine == "autograd" and res.steps == 3
    assert (seen["tr"].loss, seen["tr"].bce_target_threshold, seen["tr"].bce_sum_classes) == ("bce", 0.2, False)
    assert math.isfinite(res.history[-1]["train_loss"]) and res.history[-1]["train_loss"] > 0
    cfg.data.loss = "ce"  # the threshold is left set: refused before any engine is built
    with pytest.raises(ValueError, match="bce"):
        E.train(cfg, model=Tiny4(), train_dataset=SyntheticImages(12, 4, 3, 5, seed=1, transform=to_tensor),
                log_mlflow=False)


class Tiny4(Tiny):
    pass
