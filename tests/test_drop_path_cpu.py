"""Stochastic depth (per batch) in the native training step, on the CPU reference ops: the probability rule and
the gate values, the draws, the gate-scaling op's definition, every refusal, that rate 0 changes nothing, the
gated program against an ungated one with host-scaled BatchNorm parameters, train() and two gloo ranks."""
import copy

import numpy as np
import pytest
import torch

from dbx_distributed_pytorch_examples_amd import config as C
from dbx_distributed_pytorch_examples_amd.launch import Launcher
from dbx_distributed_pytorch_examples_amd.ops import kernels as K
from dbx_distributed_pytorch_examples_amd.ops import reference as R

pytestmark = pytest.mark.timeout(600)

CPU = torch.device("cpu")


def _batches(n, batch=4, size=32, classes=10, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randint(0, 256, (batch, size, size, 3), dtype=torch.uint8, generator=g),
             torch.randint(0, classes, (batch,), generator=g)) for _ in range(n)]


def _trainer(model=None, **kw):
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig
    from dbx_distributed_pytorch_examples_amd.models import build_model
    if model is None:
        torch.manual_seed(0)
        model = build_model("resnet18", num_classes=10)
    kw.setdefault("optim", OptimConfig(lr=0.05))
    return NativeTrainer(model, 4, (32, 32), CPU, use_graphs=False, **kw)


# ---------------------------------------------------------------------------------------------
# the rule, the gates, the draws
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,L", [(0.05, 16), (0.1, 8), (0.5, 2), (0.0, 16)])
def test_linear_rule_is_exact(rate, L):
    p = C.drop_path_probs(rate, L)
    assert len(p) == L and p[0] == 0.0
    assert p == [rate * l / (L - 1) for l in range(L)]  # float64, this expression, nothing rounded on the way
    assert all(a <= b for a, b in zip(p, p[1:])) and all(0.0 <= q < 1.0 for q in p)
    assert C.drop_path_probs(rate, 1) == [0.0]


def test_gate_values_and_the_draw_that_decides():
    seed, rate = 5, 0.4
    tr = _trainer(drop_path_rate=rate, seed=seed)
    p = tr.prog
    assert tr.drop_path_p == C.drop_path_probs(rate, 8) and p.drop_blocks == list(range(1, 8))  # first block: never
    assert p.drop_gates.dtype == torch.float32 and torch.equal(p.drop_gates, torch.ones(7))
    pl = np.array(tr.drop_path_p[1:], dtype=np.float64)
    keep = [float(np.float32(1.0 / (1.0 - q))) for q in pl]
    rng = np.random.default_rng([seed, 0x6470])  # the trainer's generator: seed + 7919 * rank, and its own stream
    seen = set()
    for x, y in _batches(6):
        tr.step(x, y)
        u = rng.random(7)
        d = tr.last_drop_path
        assert d["p"] == pl.tolist()
        assert d["dropped"] == [l + 1 for l in range(7) if u[l] < pl[l]]  # u < p_l, nothing else
        assert d["gates"] == [0.0 if u[l] < pl[l] else keep[l] for l in range(7)]
        assert p.drop_gates.tolist() == d["gates"]  # what the step's launches read
        seen.add(tuple(d["dropped"]))
    assert len(seen) > 1 and any(seen)  # the gates move from step to step, and blocks were dropped
    s = tr.drop_path_summary()
    assert (s["drop_path_rate"], s["mode"], s["blocks"], s["gated_blocks"], s["launches_per_step"]) == \
        (rate, "batch", 8, 7, 5)


def test_mix_sampler_draws_are_untouched():
    a = _trainer(cutmix_alpha=1.0, mixup_alpha=0.2, erase_prob=0.25, seed=3)
    b = _trainer(cutmix_alpha=1.0, mixup_alpha=0.2, erase_prob=0.25, seed=3, drop_path_rate=0.3)
    for x, y in _batches(4):
        a.step(x, y)
        b.step(x, y)
        da, db = a.last_mix, b.last_mix
        assert np.array_equal(da.perm, db.perm) and list(da.box) == list(db.box)
        assert (da.lam, da.blend) == (db.lam, db.blend)
        assert (da.erase is None and db.erase is None) or np.array_equal(da.erase, db.erase)
    assert b.last_drop_path is not None and a.last_drop_path is None


# ---------------------------------------------------------------------------------------------
# the op
# ---------------------------------------------------------------------------------------------
def test_reference_gate_scale_multi():
    g = torch.Generator().manual_seed(0)
    lens = [1, 3, 4, 16, 63, 64, 65, 2048]
    gates = torch.tensor([0.0, 1.0, float(np.float32(1 / 0.95))])
    src = [torch.randn(n, generator=g) for n in lens]
    dst = [torch.full((n,), 7.0) for n in lens]
    inpl = [torch.randn(n, generator=g) for n in lens]
    inpl0 = [t.clone() for t in inpl]
    rows = [(d, s, i % 3) for i, (d, s) in enumerate(zip(dst, src))] + \
           [(t, t, (i + 1) % 3) for i, t in enumerate(inpl)]  # dst == src
    desc = K.pack_gate_desc(rows, "cpu", 3)
    assert desc.dtype == torch.int64 and tuple(desc.shape) == (16, 4)
    K.gate_scale_multi(desc, 16, max(lens), gates)  # (CPU tensors: the dispatcher runs the reference)
    for i, (d, s) in enumerate(zip(dst, src)):
        assert torch.equal(d.view(torch.int32), (gates[i % 3] * s).view(torch.int32)), i
    for i, (t, t0) in enumerate(zip(inpl, inpl0)):
        assert torch.equal(t.view(torch.int32), (gates[(i + 1) % 3] * t0).view(torch.int32)), i


def test_gate_scale_refuses_before_any_launch():
    x, y = torch.zeros(8), torch.zeros(8)
    gates = torch.ones(2)
    with pytest.raises(TypeError):
        K.pack_gate_desc([(x.double(), y.double(), 0)], "cpu", 2)
    with pytest.raises(ValueError, match="rows"):
        K.pack_gate_desc([], "cpu", 2)
    with pytest.raises(ValueError, match="rows"):
        K.pack_gate_desc([(x, y, 0)] * 65536, "cpu", 2)
    with pytest.raises(ValueError, match="elements"):
        K.pack_gate_desc([(x, y[:4], 0)], "cpu", 2)
    with pytest.raises(ValueError, match="elements"):
        K.pack_gate_desc([(x[:0], y[:0], 0)], "cpu", 2)
    for bad in (-1, 2):
        with pytest.raises(ValueError, match="gate index"):
            K.pack_gate_desc([(x, y, bad)], "cpu", 2)
    with pytest.raises(ValueError, match="contiguous"):
        K.pack_gate_desc([(torch.zeros(8, 2)[:, 0], y, 0)], "cpu", 2)
    desc = K.pack_gate_desc([(x, y, 1)], "cpu", 2)
    for ref in (K.gate_scale_multi, R.gate_scale_multi):
        with pytest.raises(TypeError):
            ref(desc.int(), 1, 8, gates)
        with pytest.raises(TypeError):
            ref(desc, 1, 8, gates.double())
        with pytest.raises(ValueError):
            ref(desc, 2, 8, gates)   # the table has one row
        with pytest.raises(ValueError):
            ref(desc, 0, 8, gates)
        with pytest.raises(ValueError):
            ref(desc, 1, 0, gates)
        with pytest.raises(ValueError):
            ref(desc, 1, 8, gates[:1])  # gate index 1 of a one-gate vector
    assert torch.equal(x, torch.zeros(8))


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [-0.01, 1.0, 1.5, float("nan"), "0.1", True, None])
def test_a_rate_outside_the_interval_is_refused(rate, monkeypatch):
    from dbx_distributed_pytorch_examples_amd.data.datasets import SyntheticImages
    from dbx_distributed_pytorch_examples_amd.models import build_model
    from dbx_distributed_pytorch_examples_amd.train import engine as E
    with pytest.raises(ValueError, match="drop_path_rate"):
        C.validate_drop_path(rate)
    cfg = C.TrainConfig(model="resnet18", num_classes=10, batch_size=4, engine="native", graphs=False)
    cfg.drop_path_rate = rate
    with pytest.raises(ValueError, match="drop_path_rate"):
        C.validate_train(cfg)
    with pytest.raises(ValueError, match="drop_path_rate"):
        _trainer(build_model("resnet18", num_classes=10), drop_path_rate=rate)
    monkeypatch.setenv("DBX_FORCE_CPU", "1")
    cfg.data.image_size = 32
    with pytest.raises(ValueError, match="drop_path_rate"):
        E.train(cfg, train_dataset=SyntheticImages(8, 32, 3, 10), log_mlflow=False)


def test_the_other_engines_refuse_the_option(monkeypatch):
    from dbx_distributed_pytorch_examples_amd.data.datasets import SyntheticImages
    from dbx_distributed_pytorch_examples_amd.engine.autograd_trainer import AutogradTrainer
    from dbx_distributed_pytorch_examples_amd.engine.frozen_trainer import FrozenFeatureTrainer
    from dbx_distributed_pytorch_examples_amd.engine.native_module import native_module
    from dbx_distributed_pytorch_examples_amd.models import FrozenBackboneClassifier, build_model
    from dbx_distributed_pytorch_examples_amd.train import engine as E
    o = C.OptimizerConfig()
    with pytest.raises(ValueError, match="drop_path_rate"):
        AutogradTrainer(build_model("resnet18", num_classes=10), CPU, o, drop_path_rate=0.05)
    with pytest.raises(ValueError, match="drop_path_rate"):
        FrozenFeatureTrainer(FrozenBackboneClassifier("resnet18", num_classes=10), 4, (32, 32), CPU, o,
                             drop_path_rate=0.05)
    with pytest.raises(ValueError, match="drop_path_rate"):
        native_module(build_model("resnet18", num_classes=10), 4, (32, 32), CPU, drop_path_rate=0.05)
    for bad in (1.0, -0.5):  # (a bad rate is a bad rate there too)
        with pytest.raises(ValueError, match="drop_path_rate"):
            native_module(build_model("resnet18", num_classes=10), 4, (32, 32), CPU, drop_path_rate=bad)
    AutogradTrainer(build_model("resnet18", num_classes=10), CPU, o, drop_path_rate=0.0)  # 0 is no option
    # train(): the autograd engine and the frozen-backbone trainer
    monkeypatch.setenv("DBX_FORCE_CPU", "1")
    cfg = C.TrainConfig(model="resnet18", num_classes=10, batch_size=4, engine="autograd", drop_path_rate=0.05)
    cfg.data.image_size = 32
    with pytest.raises(ValueError, match="autograd engine"):
        E.train(cfg, train_dataset=SyntheticImages(8, 32, 3, 10), log_mlflow=False)
    cfg.engine = "native"
    with pytest.raises(ValueError, match="frozen-backbone"):
        E.train(cfg, model=FrozenBackboneClassifier("resnet18", num_classes=10),
                train_dataset=SyntheticImages(8, 32, 3, 10), log_mlflow=False)
    p = _trainer().prog
    with pytest.raises(ValueError, match="probabilities for 8 blocks"):
        p.enable_drop_path([0.0, 0.1])
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        p.enable_drop_path([0.0] * 7 + [1.0])


# ---------------------------------------------------------------------------------------------
# the program
# ---------------------------------------------------------------------------------------------
def _count_launches(monkeypatch):
    calls = []
    real = K.gate_scale_multi

    def spy(desc, nrows, max_len, gates):
        calls.append(int(nrows))
        return real(desc, nrows, max_len, gates)
    monkeypatch.setattr(K, "gate_scale_multi", spy)
    return calls


def test_rate_zero_allocates_nothing_and_launches_nothing(monkeypatch):
    calls = _count_launches(monkeypatch)
    torch.manual_seed(0)
    from dbx_distributed_pytorch_examples_amd.models import build_model
    m = build_model("resnet18", num_classes=10)
    a, b = _trainer(copy.deepcopy(m)), _trainer(copy.deepcopy(m), drop_path_rate=0.0)
    for tr in (a, b):
        p = tr.prog
        assert p.drop_gates is None and p.drop_eff is None and p._gate_fwd is None and p._gate_bwd == {}
        assert p.drop_blocks == [] and tr._drop_rng is None and tr._drop_dev is None
        assert all(bn.gamma_t is bn.gamma and bn.beta_t is bn.beta for bn in p.bns)
    for x, y in _batches(2):
        a.step(x, y)
        b.step(x, y)
    assert calls == [] and b.last_drop_path is None
    assert torch.equal(a.prog.master, b.prog.master)
    assert b.drop_path_summary()["gated_blocks"] == 0 and b.drop_path_summary()["launches_per_step"] == 0


def test_five_launches_a_step_and_the_readers_take_the_gated_copies(monkeypatch):
    calls = _count_launches(monkeypatch)
    tr = _trainer(drop_path_rate=0.2, grad_accum=2)
    p = tr.prog
    gated = [p.blocks[l].bns[-1] for l in p.drop_blocks]
    for bn in p.bns:
        on = any(bn is g for g in gated)
        assert (bn.gamma_t is not bn.gamma) == on and (bn.beta_t is not bn.beta) == on
        if on:  # views of the program's own buffer, 16-byte aligned; the master stays where the optimizer reads it
            assert bn.gamma_t.data_ptr() % 16 == 0 and bn.beta_t.data_ptr() % 16 == 0
            assert bn.gamma.data_ptr() == p.master[bn.off_w:].data_ptr()
    (x, y), = _batches(1)
    tr.step(x, y)  # a micro-step draws and launches like any other
    assert calls == [14, 4, 4, 4, 2]  # forward: 7 x (gamma, beta); backward: layer4, 3, 2 (two BNs), layer1 (one)
    tr.step(x, y)
    assert len(calls) == 10
    n = len(calls)
    tr.evaluate_batch(x, y)  # evaluation is never gated
    tr.eval_begin()
    tr.eval_step(x, y)
    tr.eval_end()
    assert len(calls) == n


def _randomised(seed=0):
    from dbx_distributed_pytorch_examples_amd.models import build_model
    torch.manual_seed(seed)
    m = build_model("resnet18", num_classes=10)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.uniform_(-0.2, 0.2)
    return m


def _one_step(model, probs=None, gates=None, host_scale=None):
    """One training step at fixed gates (written into the program directly; the trainer draws none)."""
    tr = _trainer(model)
    p = tr.prog
    if probs is not None:
        p.enable_drop_path(probs)
        p.drop_gates.copy_(torch.tensor(gates, dtype=torch.float32))
    for l, gt in (host_scale or {}).items():
        bn = p.blocks[l].bns[-1]
        bn.gamma.mul_(torch.tensor(gt, dtype=torch.float32))
        bn.beta.mul_(torch.tensor(gt, dtype=torch.float32))
    (x, y), = _batches(1)
    tr.step(x, y)
    return tr


def test_gated_program_on_the_reference_ops():
    m = _randomised()
    probs = C.drop_path_probs(0.3, 8)
    plain = _one_step(copy.deepcopy(m))
    ones = _one_step(copy.deepcopy(m), probs, [1.0] * 7)
    for a, b in ((plain.prog.logits, ones.prog.logits), (plain.prog.grad, ones.prog.grad),
                 (plain.prog.master, ones.prog.master), (plain.prog.metrics, ones.prog.metrics)):
        assert torch.equal(a, b)
    gates = [float(np.float32(1 / (1 - q))) for q in probs[1:]]
    gates[0] = gates[3] = gates[4] = 0.0  # blocks 1 (identity shortcut), 4 (downsample), 5 (identity)
    on = _one_step(copy.deepcopy(m), probs, gates)
    off = _one_step(copy.deepcopy(m), host_scale={l + 1: g for l, g in enumerate(gates)})
    p, q = on.prog, off.prog
    assert torch.equal(p.logits, q.logits) and torch.equal(p.metrics, q.metrics)
    other = torch.ones_like(p.grad, dtype=torch.bool)
    for k, l in enumerate(p.drop_blocks):
        bn, bm = p.blocks[l].bns[-1], q.blocks[l].bns[-1]
        gt = torch.tensor(gates[k], dtype=torch.float32)
        assert torch.equal(bn.dgamma.view(torch.int32), (gt * bm.dgamma).view(torch.int32)), l
        assert torch.equal(bn.dbeta.view(torch.int32), (gt * bm.dbeta).view(torch.int32)), l
        assert bool(bm.dgamma.abs().max() > 0)
        other[bn.off_w:bn.off_w + bn.C] = False
        other[bn.off_b:bn.off_b + bn.C] = False
    assert torch.equal(p.grad[other], q.grad[other])
    for (n1, b1), (_, b2) in zip(p.model.named_buffers(), q.model.named_buffers()):
        assert torch.equal(b1, b2), n1
    for l in (1, 5):  # a dropped identity block hands its input on, and nothing in it gets a gradient
        blk = p.blocks[l]
        assert blk.ds_conv is None and torch.equal(blk.out, p.blocks[l - 1].out)
        for cv in blk.convs:
            assert not bool(cv.grad.any()), cv.name
        for bn in blk.bns:
            assert not bool(bn.dgamma.any()) and not bool(bn.dbeta.any()), bn.name
    assert bool(p.blocks[2].convs[0].grad.any())  # (a kept block's do)


def test_accumulation_window_sums_differently_gated_micro_steps():
    m = _randomised(1)
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import OptimConfig
    o = OptimConfig(lr=0.0, momentum=0.0, weight_decay=0.0)
    win = _trainer(copy.deepcopy(m), optim=o, grad_accum=2, drop_path_rate=0.4, seed=5)
    one = _trainer(copy.deepcopy(m), optim=o, drop_path_rate=0.4, seed=5)
    data = _batches(2)
    gs, gates = [], []
    for x, y in data:
        one.step(x, y)
        gs.append(one.prog.grad.clone())
        win.step(x, y)
        gates.append(win.last_drop_path["gates"])
        assert win.last_drop_path == one.last_drop_path
    assert gates[0] != gates[1]
    assert torch.equal(win.prog.grad, gs[1] + gs[0])


# ---------------------------------------------------------------------------------------------
# train()
# ---------------------------------------------------------------------------------------------
def test_train_runs_on_the_cpu_with_the_native_engine(monkeypatch, tmp_path, capsys):
    from dbx_distributed_pytorch_examples_amd.data.datasets import SyntheticImages
    from dbx_distributed_pytorch_examples_amd.train import engine as E
    monkeypatch.setenv("DBX_FORCE_CPU", "1")
    monkeypatch.setenv("DBX_MLRUNS", str(tmp_path / "mlruns"))
    cfg = C.TrainConfig(model="resnet18", num_classes=10, batch_size=4, epochs=2, log_every=0, engine="native",
                        graphs=False, drop_path_rate=0.3, checkpoint_dir=str(tmp_path / "ck"))
    cfg.data.image_size = 32
    cfg.data.num_workers = 1
    cfg.optim.lr = 0.02
    seen = {}
    real = E._Native

    def spy(*a, **kw):
        r = real(*a, **kw)
        seen["tr"] = r.tr
        return r
    monkeypatch.setattr(E, "_Native", spy)
    res = E.train(cfg, train_dataset=SyntheticImages(8, 32, 3, 10), eval_dataset=SyntheticImages(6, 32, 3, 10, seed=9),
                  log_mlflow=False)
    tr = seen["tr"]
    assert res.engine == "native" and res.steps == 4 and tr.drop_path_rate == 0.3
    assert tr.last_drop_path is not None and len(tr.last_drop_path["gates"]) == 7
    assert all(h["train_loss"] == h["train_loss"] for h in res.history) and "val_accuracy" in res.history[-1]
    out = capsys.readouterr().out
    assert out.count("[train] stochastic depth:") == 1 and "drop_path_rate=0.3" in out and "mode=batch" in out
    st = torch.load(tmp_path / "ck" / "checkpoint-2.pth.tar", map_location="cpu", weights_only=True)
    assert not any("drop" in k for k in (st.get("trainer") or {}))  # no generator state, like the mix sampler's
    assert all(torch.isfinite(v).all() for v in st["model"].values() if v.is_floating_point())
    assert '"drop_path_rate": 0.3' in st["config"]


# ---------------------------------------------------------------------------------------------
# two ranks
# ---------------------------------------------------------------------------------------------
def _two_ranks():
    import torch.distributed as dist

    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig
    from dbx_distributed_pytorch_examples_amd.models import build_model
    from dbx_distributed_pytorch_examples_amd.parallel import dist as ddist
    ddist.init_distributed(device="cpu")
    rank = ddist.get_rank()
    torch.manual_seed(0)
    tr = NativeTrainer(build_model("resnet18", num_classes=4), 4, (32, 32), CPU,
                       optim=OptimConfig(lr=0.05, momentum=0.9, weight_decay=5e-4), use_graphs=False,
                       bucket_cap_mb=1.0, drop_path_rate=0.4, seed=2)
    gates = []
    for x, y in _batches(3, classes=4, seed=10 + rank):
        tr.step(x, y)
        gates.append(tr.last_drop_path["gates"])
    masters = [torch.empty_like(tr.prog.master) for _ in range(2)]
    dist.all_gather(masters, tr.prog.master)
    both = [None, None]
    dist.all_gather_object(both, gates)
    ddist.destroy()
    return {"in_sync": torch.equal(masters[0], masters[1]), "gates": both,
            "finite": bool(torch.isfinite(masters[0]).all())}


def test_two_gloo_ranks_with_different_gates_stay_in_sync():
    out = Launcher(2, use_gpu=False).run(_two_ranks)
    assert out["gates"][0] != out["gates"][1]  # seeded by seed AND rank
    assert any(0.0 in g for g in out["gates"][0] + out["gates"][1])
    assert out["in_sync"] and out["finite"]
