"""Parameter groups in the native training step, on the GPU: one eager step against the float64 formula,
graph replay following the lr schedule per group, parameters held still, a trivial table against no table
(bit for bit, on every optimizer path that takes the table), and the refusals.

Models: ``cifar_resnet18`` at 32x32, batch 16, and ResNet-50 at 32x32, batch 8 (the bottleneck layout).
The oracle and its bounds are tests/test_param_groups_cpu.py's ``step_oracle`` (the per-element bounds of
tests/test_nn_ops.py with ``lr -> f32(lr) * f32(lr_mult)``, ``wd -> f32(wd_r)``).
"""
import copy
import fnmatch

import pytest
import torch

from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig
from dbx_distributed_pytorch_examples_amd.models import build_model
from test_param_groups import report_ratios
from test_param_groups_cpu import NBD_FC10, batch, optim_for, steps_against_oracle

pytestmark = pytest.mark.gpu
MODELS = [("cifar_resnet18", 16), ("resnet50", 8)]


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    report_ratios()


def dev():
    return torch.device("cuda:0")


def trainer(arch, bsz, optim, model=None, **kw):
    if model is None:
        torch.manual_seed(0)
        model = build_model(arch, num_classes=10)
    return NativeTrainer(model, bsz, (32, 32), dev(), optim=optim, **kw)


@pytest.mark.parametrize("name", ["sgd", "adamw"])
@pytest.mark.parametrize("arch,bsz", MODELS)
def test_one_eager_step_matches_oracle(arch, bsz, name):
    """norm / bias decay 0 and fc at 10x the lr: master and moments after one eager step against the float64
    formula applied to ``prog.grad`` and the state saved before the step."""
    tr = steps_against_oracle(arch, bsz, name, "cuda", 1)
    assert tr.step_count == 1


@pytest.mark.parametrize("name", ["sgd", "adamw"])
@pytest.mark.parametrize("arch,bsz", MODELS)
def test_graph_replay_follows_the_schedule_per_group(arch, bsz, name):
    """Graphs against eager, same seed and inputs, a different lr at each of 5 steps: the masters are
    bit-identical after every step (lr is read from the device and multiplied per run in the kernel)."""
    torch.manual_seed(0)
    m1 = build_model(arch, num_classes=10)
    m2 = copy.deepcopy(m1)
    t1 = trainer(arch, bsz, optim_for(name, **NBD_FC10), model=m1, use_graphs=True)
    t2 = trainer(arch, bsz, optim_for(name, **NBD_FC10), model=m2, use_graphs=False)
    x, y = batch(bsz, 32, 10, 5, dev())
    base = t1.opt.lr
    for i, f in enumerate((1.0, 0.5, 0.7, 0.1, 0.3)):
        w = t1.prog.master.clone()
        for t in (t1, t2):
            t.set_lr(base * f)
            t.step(x, y)
        assert torch.equal(t1.prog.master, t2.prog.master), i
        assert not torch.equal(t1.prog.master, w), i
    assert len(t1.graphs) >= 1 and all(g is not None for g in t1.graphs) and not t2.graphs


@pytest.mark.parametrize("name", ["sgd", "adamw"])
@pytest.mark.parametrize("arch,bsz", MODELS)
def test_parameters_held_still(arch, bsz, name):
    """lr_mult 0 and weight_decay 0 on the stem and layer1: after 3 steps those slices of the master are
    bit-unchanged and every other tensor has changed."""
    pats = ["conv1.*", "bn1.*", "layer1.*"]
    tr = trainer(arch, bsz, optim_for(name, groups=[{"match": pats, "lr_mult": 0, "weight_decay": 0}]))
    w0 = tr.prog.master.clone()
    x, y = batch(bsz, 32, 10, 2, dev())
    for _ in range(3):
        tr.step(x, y)
    held = 0
    for pname, off, n in tr.prog.param_ranges:
        same = torch.equal(tr.prog.master[off:off + n].view(torch.int32), w0[off:off + n].view(torch.int32))
        if any(fnmatch.fnmatchcase(pname, p) for p in pats):
            assert same, f"{pname} moved"
            held += 1
        else:
            assert not same, f"{pname} did not change"
    assert held >= 3 and held < len(tr.prog.param_ranges)


TRIVIAL = [dict(), dict(grad_clip=0.5), dict(ema_decay=0.9), dict(grad_accum=2), dict(overlap=True)]


@pytest.mark.parametrize("variant", TRIVIAL, ids=["plain", "clip", "ema", "accum2", "overlap"])
@pytest.mark.parametrize("name", ["sgd", "adamw"])
def test_trivial_table_equals_no_table(name, variant, engine):
    """Explicit groups whose values equal the defaults: after 3 optimizer steps the master (and the weight
    average) is bit-identical to a trainer built without groups -- on the plain and the clipped optimizer
    phase, with the fused EMA, with gradient accumulation and with the optimizer inside the backward."""
    v = dict(variant)
    clip, ema, accum, overlap = v.get("grad_clip", 0.0), v.get("ema_decay", 0.0), v.get("grad_accum", 1), v.get("overlap")
    arch, bsz = "cifar_resnet18", 16
    torch.manual_seed(0)
    m1 = build_model(arch, num_classes=10)
    m2 = copy.deepcopy(m1)
    wd = optim_for(name).weight_decay
    groups = [{"match": "layer*", "weight_decay": wd, "lr_mult": 1.0}, {"match": "*", "lr_mult": 1}]
    if overlap:
        engine(overlap_optimizer=-1)  # every backward segment's update right behind it: _update_range(lo, hi)
    kw = dict(ema_decay=ema, grad_accum=accum, use_graphs=True)
    t1 = trainer(arch, bsz, optim_for(name, grad_clip=clip, groups=groups, norm_weight_decay=wd), model=m1, **kw)
    t2 = trainer(arch, bsz, optim_for(name, grad_clip=clip), model=m2, **kw)
    assert t1.group_runs is not None and t2.group_runs is None
    assert len(t1.group_runs._dbx_runs[2]) == 1  # merged into one run
    if overlap:
        assert t1.opt_ranges is not None and t2.opt_ranges is not None
    data = [batch(bsz, 32, 10, s, dev()) for s in (1, 2)]
    w0 = t1.prog.master.clone()
    for i in range(3 * accum):
        for t in (t1, t2):
            t.step(*data[i % 2])
    assert t1.step_count == t2.step_count == 3
    assert torch.equal(t1.prog.master, t2.prog.master) and not torch.equal(t1.prog.master, w0)
    assert torch.equal(t1.mom, t2.mom)
    if ema:
        assert torch.equal(t1.ema, t2.ema) and not torch.equal(t1.ema, t1.prog.master)


@pytest.mark.parametrize("kw", [dict(name="lars"), dict(name="lamb"), dict(name="sgd", zero_stage=1)],
                         ids=["lars", "lamb", "zero1"])
def test_refusals(kw):
    kw = dict(kw)
    zs = kw.pop("zero_stage", 0)
    with pytest.raises(ValueError, match="[Pp]arameter groups"):
        trainer("cifar_resnet18", 16, OptimConfig(groups=[{"match": "fc.*", "lr_mult": 10}], **kw), zero_stage=zs)


@pytest.mark.parametrize("name", ["sgd", "adamw"])
def test_optimizer_in_backward_reads_the_whole_buffers_table(name, engine):
    """The optimizer inside the backward updates slices [lo, hi) of the master with ``run_base=lo`` into the
    one table: with real groups (a dozen runs) it equals the single update at the end of the step, bit for bit."""
    torch.manual_seed(0)
    m1 = build_model("resnet50", num_classes=10)
    m2 = copy.deepcopy(m1)
    engine(overlap_optimizer=-1)
    t1 = trainer("resnet50", 8, optim_for(name, **NBD_FC10), model=m1)
    engine(overlap_optimizer=0)
    t2 = trainer("resnet50", 8, optim_for(name, **NBD_FC10), model=m2)
    assert t1.opt_ranges is not None and t2.opt_ranges is None
    assert any(lo > 0 for rs in t1.opt_ranges["per_phase"] for lo, _ in rs)
    x, y = batch(8, 32, 10, 4, dev())
    for _ in range(3):
        t1.step(x, y)
        t2.step(x, y)
    assert torch.equal(t1.prog.master, t2.prog.master) and torch.equal(t1.mom, t2.mom)
