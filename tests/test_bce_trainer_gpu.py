"""Binary cross-entropy as the training loss of the native step, on the GPU: ResNet-18 with the CIFAR stem, 32x32,
10 classes, batch 8 unless stated. The step's ``dlogits`` and metrics are ``K.bce_logits`` of its own logits (with
the step's mixed labels where it mixes), a replayed graph equals the eager step, accumulation and the frozen-
backbone head see the same loss, and without the argument nothing changes."""
import copy
import math

import pytest
import torch

from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig
from dbx_distributed_pytorch_examples_amd.models import build_model
from dbx_distributed_pytorch_examples_amd.ops import kernels as K

pytestmark = pytest.mark.gpu
N, HW, CLASSES = 8, 32, 10
MIX = dict(mixup_alpha=0.2, cutmix_alpha=1.0)


def dev():
    return torch.device("cuda:0")


def trainer(model=None, batch=N, **kw):
    if model is None:
        torch.manual_seed(0)
        model = build_model("resnet18", num_classes=CLASSES)
    kw.setdefault("optim", OptimConfig(lr=0.05))
    return NativeTrainer(model, batch, (HW, HW), dev(), **kw)


def batches(n, batch=N, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randint(0, 256, (batch, HW, HW, 3), dtype=torch.uint8, generator=g).to(dev()),
             torch.randint(0, CLASSES, (batch,), generator=g).to(dev())) for _ in range(n)]


def bce_of(logits, labels, **kw):
    """(dlogits, metrics) of a direct K.bce_logits call on a copy of ``logits``."""
    lg = logits.clone()
    dl = torch.full_like(lg, float("nan"))
    st = torch.zeros(2, dtype=torch.float64, device=lg.device)
    K.bce_logits(lg, labels, dl, None, st, **kw)
    return dl, st


@pytest.mark.parametrize("opts", [dict(), dict(label_smoothing=0.1, bce_target_threshold=0.2, bce_sum_classes=True)],
                         ids=["plain", "smooth-thr-sum"])
def test_step_is_the_kernel_on_its_logits(opts):
    tr = trainer(use_graphs=False, loss="bce", **opts)
    p = tr.prog
    (img, lab), = batches(1)
    tr.step(img, lab)
    dl, st = bce_of(p.logits, lab, smoothing=opts.get("label_smoothing", 0.0),
                    target_threshold=opts.get("bce_target_threshold"), sum_classes=opts.get("bce_sum_classes", False))
    assert torch.equal(p.dlogits, dl)
    assert torch.equal(p.metrics, st) and float(st[0]) > 0
    s = tr.loss_summary()
    assert s["loss"] == "bce" and s["kernel"] == "bce_logits"
    assert s["bce_target_threshold"] == opts.get("bce_target_threshold")
    assert s["bce_sum_classes"] == opts.get("bce_sum_classes", False)


def test_step_with_mixing_is_the_kernel_on_the_mixed_labels():
    tr = trainer(use_graphs=False, loss="bce", seed=3, **MIX)
    p = tr.prog
    kinds = set()
    for img, lab in batches(4):
        tr.read_metrics()
        tr.step(img, lab)
        d = tr.last_mix
        kinds.add(d.kind)
        perm = torch.as_tensor(d.perm).to(dev()).long()
        dl, st = bce_of(p.logits, lab, labels2=lab[perm], lam=torch.tensor([d.lam], dtype=torch.float32, device=dev()))
        assert torch.equal(p.dlogits, dl), d.kind
        assert torch.equal(p.metrics, st), d.kind
    assert kinds <= {"mixup", "cutmix"} and kinds


def test_graph_replay_equals_eager():
    """Same seed, graphs on / off, MixUp and CutMix on, 4 steps (two eager warm-ups, the capture, a replay)."""
    torch.manual_seed(0)
    m1 = build_model("resnet18", num_classes=CLASSES)
    m2 = copy.deepcopy(m1)
    a = trainer(m1, seed=4, loss="bce", bce_target_threshold=0.2, use_graphs=True, **MIX)
    b = trainer(m2, seed=4, loss="bce", bce_target_threshold=0.2, use_graphs=False, **MIX)
    for i, bt in enumerate(batches(4, seed=2)):
        a.step(*bt)
        b.step(*bt)
        assert a.last_mix.lam == b.last_mix.lam
        assert torch.equal(a.prog.dlogits, b.prog.dlogits), i
        assert torch.equal(a.prog.master, b.prog.master), i
    assert a.read_metrics() == b.read_metrics()
    assert a.graphs and all(g is not None for g in a.graphs) and not b.graphs


def test_loss_falls():
    """30 Adam steps on one fixed random batch of 64 (the memorisation task of tests/test_program_gpu.py)."""
    torch.manual_seed(0)
    tr = trainer(batch=64, loss="bce", optim=OptimConfig(name="adam", lr=1e-3, weight_decay=0.0))
    g = torch.Generator().manual_seed(3)
    img = torch.randint(0, 256, (64, HW, HW, 3), dtype=torch.uint8, generator=g).to(dev())
    lab = torch.randint(0, CLASSES, (64,), generator=g).to(dev())
    losses = []
    for _ in range(30):
        tr.step(img, lab)
        losses.append(tr.read_metrics()[0] / 64)
    print("[bce loss30] " + " ".join(f"{v:.4f}" for v in losses[::5]))
    assert all(math.isfinite(v) for v in losses), losses
    assert sum(losses[-5:]) / 5 < sum(losses[:5]) / 5, losses


def test_accumulation_window():
    """grad_accum 2, eager: the boundary step's gradient is g2 + g1 of the two micro-batches, harvested from a twin
    with lr 0 and the same loss (the comparison of tests/test_grad_accum_gpu.py), and the metrics add up."""
    torch.manual_seed(0)
    model = build_model("resnet18", num_classes=CLASSES)
    twin = copy.deepcopy(model)
    kw = dict(loss="bce", label_smoothing=0.1, use_graphs=False)
    tr = trainer(model, grad_accum=2, optim=OptimConfig(lr=0.05, momentum=0.9, weight_decay=5e-4), **kw)
    th = trainer(twin, optim=OptimConfig(lr=0.0, momentum=0.0, weight_decay=0.0), **kw)
    init = tr.prog.master.clone()
    data = batches(2)
    gs, dls = [], []
    for x, y in data:
        th.step(x, y)
        gs.append(th.prog.grad.clone())
        dls.append(th.prog.dlogits.clone())
    for i, (x, y) in enumerate(data):
        tr.step(x, y)
        assert torch.equal(tr.prog.dlogits, dls[i]), i
        if i == 0:
            assert torch.equal(tr.prog.master, init)
    assert tr.step_count == 1 and tr.micro == 0
    assert torch.equal(tr.prog.grad, gs[1] + gs[0])
    assert not torch.equal(tr.prog.master, init)
    assert tr.read_metrics() == th.read_metrics()


def test_frozen_head_uses_the_kernel():
    from dbx_distributed_pytorch_examples_amd.config import OptimizerConfig
    from dbx_distributed_pytorch_examples_amd.engine.frozen_trainer import FrozenFeatureTrainer
    from dbx_distributed_pytorch_examples_amd.models import FrozenBackboneClassifier
    torch.manual_seed(1)
    m = FrozenBackboneClassifier("resnet18", num_classes=CLASSES)
    tr = FrozenFeatureTrainer(m, N, (HW, HW), dev(), OptimizerConfig(name="adam", lr=1e-3), label_smoothing=0.1,
                              use_graphs=False, loss="bce", bce_target_threshold=0.2)
    assert tr.nhead is not None and tr.nhead.loss == "bce"
    (img, lab), = batches(1)
    tr.step(img, lab)
    dl, st = bce_of(tr.nhead.logits, lab, smoothing=0.1, target_threshold=0.2)
    assert torch.equal(tr.nhead.dlogits, dl)
    assert torch.equal(tr.metrics64, st)
    with pytest.raises(ValueError):
        FrozenFeatureTrainer(m, N, (HW, HW), dev(), OptimizerConfig(name="adam", lr=1e-3), bce_sum_classes=True)


def test_default_is_softmax_ce():
    """Without the argument and with loss="ce": the same metrics and master after 2 steps, and no BCE launch."""
    torch.manual_seed(0)
    m1 = build_model("resnet18", num_classes=CLASSES)
    m2 = copy.deepcopy(m1)
    a, b = trainer(m1, use_graphs=False), trainer(m2, use_graphs=False, loss="ce")
    assert a.loss_summary()["kernel"] == "softmax_ce" and a.prog.loss_kind == "ce"
    for bt in batches(2):
        a.step(*bt)
        b.step(*bt)
    dl = torch.full_like(a.prog.dlogits, float("nan"))
    K.softmax_ce(a.prog.logits.clone(), batches(2)[1][1], dl)
    assert torch.equal(a.prog.dlogits, dl)
    assert a.read_metrics() == b.read_metrics()
    assert torch.equal(a.prog.master, b.prog.master)
    for bad in (dict(loss="focal"), dict(bce_target_threshold=0.2), dict(loss="ce", bce_sum_classes=True),
                dict(loss="bce", bce_target_threshold=1.0)):
        with pytest.raises(ValueError):
            trainer(copy.deepcopy(m1), **bad)
