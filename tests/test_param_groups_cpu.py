"""Parameter groups above the kernels, without a GPU: resolution (config.resolve_param_groups), the input
forms, run merging on a real program, the native trainer on the CPU reference path against the float64
formula, the autograd engine's torch param groups, and the refusals.

The trainer oracle (``step_oracle``) is the float64 textbook formula applied to the step's own gradient and
the state saved before the step, with per-element ``f32(wd)`` / ``f32(lr) * f32(lr_mult)`` vectors; its
bounds are tests/test_nn_ops.py's per-element bounds of ``test_sgd_step`` / ``test_adam_step`` (see
tests/test_param_groups.py). tests/test_param_groups_gpu.py imports it.
"""
import copy
import json
import os

import pytest
import torch
import torch.nn as nn

from dbx_distributed_pytorch_examples_amd import config as C
from dbx_distributed_pytorch_examples_amd.config import OptimizerConfig, load_config, resolve_param_groups
from dbx_distributed_pytorch_examples_amd.engine.autograd_trainer import (LAMB, LARS, AutogradTrainer,
                                                                           build_torch_optimizer, param_kinds)
from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig
from dbx_distributed_pytorch_examples_amd.engine.program import ResNetProgram
from dbx_distributed_pytorch_examples_amd.models import build_model
from test_nn_ops import f32, f32_bound
from test_param_groups import check, report_ratios

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [("conv1.weight", "weight"), ("bn1.weight", "norm"), ("bn1.bias", "norm"),
         ("layer1.0.conv1.weight", "weight"), ("layer1.0.bn1.weight", "norm"), ("fc.weight", "weight"),
         ("fc.bias", "bias")]


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    report_ratios()


def O(**kw):
    return OptimizerConfig(weight_decay=5e-5, **kw)


# ---------------------------------------------------------------------------------------------
# resolution
# ---------------------------------------------------------------------------------------------
def test_nothing_set_is_no_table():
    assert resolve_param_groups(NAMES, O()) is None
    assert not C.has_param_groups(O())
    assert C.has_param_groups(O(norm_weight_decay=0.0)) and C.has_param_groups(O(groups=[{"match": "fc.*"}]))


def test_shorthands():
    got = resolve_param_groups(NAMES, O(norm_weight_decay=0.0, bias_weight_decay=1e-3))
    assert got == [(5e-5, 1.0), (0.0, 1.0), (0.0, 1.0), (5e-5, 1.0), (0.0, 1.0), (5e-5, 1.0), (1e-3, 1.0)]
    got = resolve_param_groups(NAMES, O(bias_weight_decay=0.0))  # BN biases are "norm", not "bias"
    assert got == [(5e-5, 1.0)] * 6 + [(0.0, 1.0)]


def test_order_and_first_match():
    groups = [{"match": "fc.bias", "weight_decay": 0.5, "lr_mult": 3.0},
              {"match": ["fc.*", "layer1.*"], "weight_decay": 0.25, "lr_mult": 2.0},
              {"match": "*", "lr_mult": 0.5}]
    got = dict(zip([n for n, _ in NAMES], resolve_param_groups(NAMES, O(groups=groups))))
    assert got["fc.bias"] == (0.5, 3.0)                 # the first match wins, not the last or the widest
    assert got["fc.weight"] == got["layer1.0.conv1.weight"] == got["layer1.0.bn1.weight"] == (0.25, 2.0)
    assert got["conv1.weight"] == (5e-5, 0.5) and got["bn1.weight"] == (5e-5, 0.5)
    got = resolve_param_groups(NAMES, O(groups=list(reversed(groups))))
    assert set(got) == {(5e-5, 0.5)}                    # "*" first: nothing else is reached


def test_fall_through_per_key():
    o = O(norm_weight_decay=0.0, bias_weight_decay=1e-3,
          groups=[{"match": "fc.*", "lr_mult": 10}, {"match": "bn1.*", "weight_decay": 0.125}])
    got = dict(zip([n for n, _ in NAMES], resolve_param_groups(NAMES, o)))
    assert got["fc.weight"] == (5e-5, 10.0)   # weight_decay missing -> the default
    assert got["fc.bias"] == (1e-3, 10.0)     # ... -> the bias shorthand
    assert got["bn1.weight"] == (0.125, 1.0)  # lr_mult missing -> 1.0; the group's decay beats the shorthand
    assert got["layer1.0.bn1.weight"] == (0.0, 1.0)
    # a group's weight_decay is absolute, as torch's: 0 means 0
    got = dict(zip([n for n, _ in NAMES], resolve_param_groups(NAMES, O(groups=[{"match": "conv1.*", "weight_decay": 0}]))))
    assert got["conv1.weight"] == (0.0, 1.0)


@pytest.mark.parametrize("groups,exc", [
    ([{"match": "nothing.*", "lr_mult": 2}], ValueError),
    ([{"match": "fc.*", "lr_mult": -1}], ValueError),
    ([{"match": "fc.*", "weight_decay": -1e-3}], ValueError),
    ([{"match": "fc.*", "lr_mult": float("nan")}], ValueError),
    ([{"match": "fc.*", "weight_decay": float("inf")}], ValueError),
    ([{"match": "fc.*", "lr": 0.1}], KeyError),
    ([{"match": "fc.*", "lr_mult": 1, "momentum": 0.5}], KeyError),
    ([{"lr_mult": 2}], ValueError),
])
def test_resolution_errors(groups, exc):
    with pytest.raises(exc):
        resolve_param_groups(NAMES, O(groups=groups))


def test_non_finite_shorthand_raises():
    with pytest.raises(ValueError):
        resolve_param_groups(NAMES, O(norm_weight_decay=float("nan")))
    with pytest.raises(ValueError):
        resolve_param_groups(NAMES, O(bias_weight_decay=float("inf")))


# ---------------------------------------------------------------------------------------------
# input forms
# ---------------------------------------------------------------------------------------------
def test_yaml_cli_json_forms(tmp_path):
    y = tmp_path / "c.yaml"
    y.write_text("model: resnet18\noptim:\n  name: sgd\n  norm_weight_decay: 0\n  groups:\n"
                 "    - {match: 'fc.*', lr_mult: 10}\n    - match: [layer4.*, layer3.*]\n      weight_decay: 0.001\n")
    cfg = load_config(str(y))
    assert cfg.optim.norm_weight_decay == 0.0 and cfg.optim.bias_weight_decay == -1.0
    assert cfg.optim.groups == [{"match": "fc.*", "lr_mult": 10}, {"match": ["layer4.*", "layer3.*"], "weight_decay": 0.001}]
    j = tmp_path / "c.json"
    j.write_text(json.dumps({"optim": {"groups": [{"match": "fc.*", "lr_mult": 10}], "bias_weight_decay": 0}}))
    cfg = load_config(str(j))
    assert cfg.optim.groups == [{"match": "fc.*", "lr_mult": 10}] and cfg.optim.bias_weight_decay == 0.0
    cfg = load_config(None, ['optim.groups=[{"match": "fc.*", "lr_mult": 10}, {"match": ["bn1.*"], "weight_decay": 0}]',
                             "optim.norm_weight_decay=0"])
    assert cfg.optim.groups == [{"match": "fc.*", "lr_mult": 10}, {"match": ["bn1.*"], "weight_decay": 0}]
    assert cfg.optim.norm_weight_decay == 0.0
    cfg = C.update_dataclass(C.TrainConfig(), {"optim": {"groups": '[{"match": "fc.*", "lr_mult": 2}]'}})
    assert cfg.optim.groups == [{"match": "fc.*", "lr_mult": 2}]
    with pytest.raises(ValueError):
        load_config(None, ["optim.groups=3"])
    assert C.TrainConfig().optim.groups == [] and C.TrainConfig().optim.groups is not C.TrainConfig().optim.groups


def test_nbd_config_loads():
    cfg = load_config(os.path.join(ROOT, "configs", "resnet50_imagenet_8192_nbd.yaml"))
    base = load_config(os.path.join(ROOT, "configs", "resnet50_imagenet_8192.yaml"))
    assert cfg.optim.norm_weight_decay == 0.0 and cfg.optim.bias_weight_decay == 0.0 and cfg.optim.groups == []
    assert not C.has_param_groups(base.optim)
    cfg.optim.norm_weight_decay = cfg.optim.bias_weight_decay = -1.0
    assert cfg == base  # the north-star config plus the two shorthands, nothing else


# ---------------------------------------------------------------------------------------------
# names, kinds, run merging on a real program
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch,size", [("resnet18", 32), ("resnet50", 32), ("cifar_resnet18", 32)])
def test_param_ranges_names_are_named_parameters(arch, size):
    torch.manual_seed(0)
    model = build_model(arch, num_classes=10)
    names = {n for n, _ in model.named_parameters()}
    kinds = param_kinds(model)
    prog = ResNetProgram(model, 2, (size, size), torch.device("cpu"))
    assert {r[0] for r in prog.param_ranges} == names
    assert len(prog.param_ranges) == len(names)
    # the trainer's name rule and the autograd engine's module-type rule agree on every parameter
    bn = {f"{b.name}." for b in prog.bns}
    for n in names:
        k = "norm" if any(n.startswith(b) for b in bn) else "bias" if n.endswith(".bias") else "weight"
        assert kinds[n] == k, n


def test_run_merging_resnet50():
    """norm / bias decay 0 on ResNet-50: within a backward segment the conv weights come first, then the BN
    pairs, so the table is a dozen runs; the count is computed here from ``param_ranges``."""
    torch.manual_seed(0)
    tr = NativeTrainer(build_model("resnet50", num_classes=10), 2, (32, 32), torch.device("cpu"), use_graphs=False,
                       optim=OptimConfig(weight_decay=5e-5, norm_weight_decay=0.0, bias_weight_decay=0.0))
    rs = sorted(tr.prog.param_ranges, key=lambda r: r[1])
    bn = {f"{b.name}." for b in tr.prog.bns}
    decayed = [not (any(r[0].startswith(b) for b in bn) or r[0].endswith(".bias")) for r in rs]
    want = 1 + sum(a != b for a, b in zip(decayed, decayed[1:]))
    starts, wds, lms = tr.group_runs._dbx_runs[1:]
    assert len(wds) == want == 12, (len(wds), want)
    assert starts[0] == 0 and starts[-1] == tr.prog.n_params and all(s % 16 == 0 for s in starts)
    assert set(wds) == {0.0, 5e-5} and set(lms) == {1.0}
    assert all(a != b for a, b in zip(wds, wds[1:]))  # merged: no equal neighbours
    # every tensor lies in one run that carries its values
    tab = {n: (wd, lm) for n, wd, lm in tr.param_group_table()}
    for (name, off, n), dec in zip(rs, decayed):
        r = max(i for i, s in enumerate(starts[:-1]) if s <= off)
        assert off + n <= starts[r + 1] and (wds[r], lms[r]) == tab[name] == ((5e-5 if dec else 0.0), 1.0)
    rows = tr.param_group_summary()
    assert [(wd, lm) for wd, lm, _, _ in rows] == [(5e-5, 1.0), (0.0, 1.0)]
    assert sum(nt for _, _, nt, _ in rows) == len(rs) and sum(ne for _, _, _, ne in rows) == sum(r[2] for r in rs)
    # one run per tensor: distinct values on neighbours are not merged
    tr2 = NativeTrainer(build_model("resnet18", num_classes=10), 2, (32, 32), torch.device("cpu"), use_graphs=False,
                        optim=OptimConfig(groups=[{"match": "*.weight", "lr_mult": 0.5}, {"match": "layer?.1.*", "lr_mult": 2}]))
    assert tr2.group_runs is not None and NativeTrainer(
        build_model("resnet18", num_classes=10), 2, (32, 32), torch.device("cpu"), use_graphs=False).group_runs is None


# ---------------------------------------------------------------------------------------------
# the native trainer on the CPU reference path
# ---------------------------------------------------------------------------------------------
def group_vectors(tr):
    """Per-element float64 (f32(wd), f32(lr_mult)) over the flat master from ``param_group_table()``; the
    alignment padding keeps (0, 0): master and gradient are zero there."""
    n = tr.prog.n_params
    wd, lm = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for (name, off, ln), (name2, w, m) in zip(tr.prog.param_ranges, tr.param_group_table()):
        assert name == name2
        wd[off:off + ln], lm[off:off + ln] = f32(w), f32(m)
    return wd.to(tr.dev), lm.to(tr.dev)


def step_oracle(tr, key, dev, w0, g, m0, v0, wdv, lmv, t, tag):
    """Check master and moments after optimizer step ``t`` (1-based) of ``tr`` (sgd with momentum, or adamw)
    from the state before it and the step's gradient ``g``; the padding must still be zero."""
    o = tr.opt
    w0, g, m0 = w0.double(), g.double(), m0.double()
    flr = f32(o.lr) * lmv
    if o.name == "sgd":
        fm = f32(o.momentum)
        d, dmag = g + wdv * w0, g.abs() + (wdv * w0).abs()
        buf, bmag = fm * m0 + d, (fm * m0).abs() + dmag
        check(key + " buf", dev, tr.mom, buf, f32_bound(bmag), tag + " buf")
        check(key + " p", dev, tr.prog.master, w0 - flr * buf, f32_bound(w0.abs() + flr * bmag), tag + " p")
        return
    b1, b2, eps = f32(o.betas[0]), f32(o.betas[1]), f32(o.eps)
    bc1, bc2 = f32(1 - o.betas[0] ** t), f32(1 - o.betas[1] ** t)
    v0 = v0.double()
    pp, pmag = w0 - flr * wdv * w0, w0.abs() + (flr * wdv * w0).abs()
    mm, mmag = b1 * m0 + (1 - b1) * g, (b1 * m0).abs() + (1 - b1) * g.abs()
    vv, vmag = b2 * v0 + (1 - b2) * g * g, (b2 * v0).abs() + 2 * (1 - b2) * g * g
    den = torch.sqrt(vv / bc2) + eps
    upd = flr * (mm / bc1) / den
    umag = flr * (mmag / bc1) / den + upd.abs() * (1 + 0.5 * vmag / vv.clamp_min(1e-300))
    check(key + " m", dev, tr.mom, mm, f32_bound(mmag), tag + " m")
    check(key + " v", dev, tr.mom2, vv, f32_bound(vmag), tag + " v")
    check(key + " p", dev, tr.prog.master, pp - upd, f32_bound(pmag + umag), tag + " p")


def batch(n, size, classes, seed, dev):
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (n, size, size, 3), dtype=torch.uint8, generator=g).to(dev)
    return img, torch.randint(0, classes, (n,), generator=g).to(dev)


NBD_FC10 = dict(norm_weight_decay=0.0, bias_weight_decay=0.0, groups=[{"match": "fc.*", "lr_mult": 10}])


def optim_for(name, **kw):
    if name == "sgd":
        return OptimConfig(name="sgd", lr=0.05, momentum=0.9, weight_decay=1e-2, **kw)
    return OptimConfig(name="adamw", lr=2e-3, weight_decay=1e-2, **kw)


def steps_against_oracle(arch, bsz, name, dev, steps):
    d = torch.device(dev if dev == "cpu" else "cuda:0")
    torch.manual_seed(0)
    model = build_model(arch, num_classes=10)
    twin = copy.deepcopy(model)
    A = NativeTrainer(model, bsz, (32, 32), d, use_graphs=False, optim=optim_for(name, **NBD_FC10))
    Bt = NativeTrainer(twin, bsz, (32, 32), d, use_graphs=False,
                       optim=OptimConfig(name="sgd", lr=0.0, momentum=0.0, weight_decay=0.0))
    assert A.group_runs is not None and Bt.group_runs is None
    tab = {n: (wd, lm) for n, wd, lm in A.param_group_table()}
    assert tab["fc.weight"] == (1e-2, 10.0) and tab["fc.bias"] == (0.0, 10.0) and tab["bn1.weight"] == (0.0, 1.0)
    assert tab["conv1.weight"] == (1e-2, 1.0)
    wdv, lmv = group_vectors(A)
    x, y = batch(bsz, 32, 10, 1, d)
    for t in range(1, steps + 1):
        w0, m0 = A.prog.master.clone(), A.mom.clone()
        v0 = A.mom2.clone() if A.mom2 is not None else None
        Bt.prog.master.copy_(w0)
        Bt.step(x, y)
        g = Bt.prog.grad.clone()  # (the program is bit-reproducible: the gradient A's step sees)
        assert torch.equal(Bt.prog.master, w0)
        A.step(x, y)
        step_oracle(A, f"trainer {name}", dev, w0, g, m0, v0, wdv, lmv, t, f"{arch} {name} step{t}")
    return A


@pytest.mark.parametrize("name", ["sgd", "adamw"])
def test_native_trainer_cpu_three_steps(name):
    steps_against_oracle("cifar_resnet18", 16, name, "cpu", 3)


# ---------------------------------------------------------------------------------------------
# autograd engine
# ---------------------------------------------------------------------------------------------
def test_autograd_engine_groups():
    torch.manual_seed(0)
    model = build_model("resnet18", num_classes=10)
    o = OptimizerConfig(name="sgd", lr=0.1, weight_decay=1e-2, norm_weight_decay=0.0, bias_weight_decay=0.0,
                        groups=[{"match": "fc.*", "lr_mult": 10}])
    tr = AutogradTrainer(model, torch.device("cpu"), o)
    gs = tr.opt.param_groups
    got = {(g["weight_decay"], g["lr_mult"]): g for g in gs}
    assert set(got) == {(1e-2, 1.0), (0.0, 1.0), (1e-2, 10.0), (0.0, 10.0)} and len(gs) == 4
    named = dict(model.named_parameters())
    assert [id(p) for p in got[(1e-2, 10.0)]["params"]] == [id(named["fc.weight"])]
    assert [id(p) for p in got[(0.0, 10.0)]["params"]] == [id(named["fc.bias"])]
    n_norm = sum(1 for n in named if param_kinds(model)[n] == "norm")
    assert len(got[(0.0, 1.0)]["params"]) == n_norm == 40
    assert sum(len(g["params"]) for g in gs) == len(named)
    assert all(g["lr"] == pytest.approx(0.1 * g["lr_mult"]) for g in gs)
    tr.set_lr(0.02)
    assert all(g["lr"] == pytest.approx(0.02 * g["lr_mult"]) for g in gs) and tr.o.lr == 0.02
    # without groups: one group, and set_lr writes the plain value
    tr = AutogradTrainer(build_model("resnet18", num_classes=10), torch.device("cpu"), OptimizerConfig(name="adamw"))
    tr.set_lr(0.3)
    assert len(tr.opt.param_groups) == 1 and tr.opt.param_groups[0]["lr"] == 0.3
    # GroupNorm / LayerNorm parameters are "norm" by module type, whatever their names
    m = nn.Sequential(nn.Linear(4, 4), nn.LayerNorm(4), nn.GroupNorm(2, 4))
    assert param_kinds(m) == {"0.weight": "weight", "0.bias": "bias", "1.weight": "norm", "1.bias": "norm",
                              "2.weight": "norm", "2.bias": "norm"}
    opt = build_torch_optimizer(list(m.named_parameters()), OptimizerConfig(name="adamw", norm_weight_decay=0.0), m)
    assert sorted(g["weight_decay"] for g in opt.param_groups) == [0.0, 5e-5]


def test_autograd_engine_refusals():
    m = nn.Linear(4, 4)
    named = list(m.named_parameters())
    for name in ("lars", "lamb"):
        with pytest.raises(ValueError, match="parameter groups"):
            build_torch_optimizer(named, OptimizerConfig(name=name, bias_weight_decay=0.0), m)
    with pytest.raises(ValueError, match="named"):
        build_torch_optimizer(list(m.parameters()), OptimizerConfig(bias_weight_decay=0.0))
    for cls in (LARS, LAMB):
        with pytest.raises(ValueError, match="parameter groups"):
            cls([{"params": [m.weight]}, {"params": [m.bias], "weight_decay": 0.0}], lr=0.1)
        cls(m.parameters(), lr=0.1)


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(name="lars"), dict(name="lamb"), dict(name="sgd", zero_stage=1)])
def test_native_trainer_refusals_cpu(kw):
    zs = kw.pop("zero_stage", 0)
    with pytest.raises(ValueError, match="[Pp]arameter groups"):
        NativeTrainer(build_model("resnet18", num_classes=10), 2, (32, 32), torch.device("cpu"), use_graphs=False,
                      zero_stage=zs, optim=OptimConfig(norm_weight_decay=0.0, **kw))


def test_sharded_optimizers_refuse():
    from dbx_distributed_pytorch_examples_amd.parallel.fsdp import ShardedDataParallel
    from dbx_distributed_pytorch_examples_amd.parallel.zero import ZeroShardedOptimizer
    o = OptimizerConfig(name="adamw", groups=[{"match": "*", "lr_mult": 0.5}])
    buf = torch.zeros(64)
    with pytest.raises(ValueError, match="parameter groups"):
        ZeroShardedOptimizer(buf, buf.clone(), o, stage=1)
    with pytest.raises(ValueError, match="parameter groups"):
        ShardedDataParallel(nn.Linear(4, 4), o)
    with pytest.raises(ValueError, match="parameter groups"):
        AutogradTrainer(nn.Linear(4, 4), torch.device("cpu"), o, zero_stage=1)


def test_train_refuses_frozen_backbone(monkeypatch):
    """A run that would use the frozen-backbone trainer refuses groups instead of ignoring them."""
    from dbx_distributed_pytorch_examples_amd.engine.frozen_trainer import FrozenFeatureTrainer
    from dbx_distributed_pytorch_examples_amd.models import FrozenBackboneClassifier
    from dbx_distributed_pytorch_examples_amd.train import engine as E
    model = FrozenBackboneClassifier("resnet18", 10)
    monkeypatch.setattr(E, "_pick_engine", lambda *a: "native")
    monkeypatch.setattr(E, "_Native", lambda *a, **k: (_ for _ in ()).throw(AssertionError("built a runner")))
    monkeypatch.setenv("DBX_FORCE_CPU", "1")
    cfg = C.TrainConfig(model="frozen_resnet18", num_classes=10, batch_size=4, max_steps=1)
    cfg.data.image_size, cfg.data.train_samples = 32, 8
    cfg.optim.bias_weight_decay = 0.0
    with pytest.raises(ValueError, match="frozen-backbone"):
        E.train(cfg, model=model, log_mlflow=False)
    with pytest.raises(ValueError, match="frozen-backbone"):
        FrozenFeatureTrainer(model, 4, (32, 32), torch.device("cpu"), cfg.optim)
