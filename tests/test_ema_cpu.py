"""Weight EMA in the native training step, on the CPU reference ops: the reference update against
float64, the decay schedule, fused trainers against twins averaged from outside, boundary-only
updates under gradient accumulation, the refused configurations, and train() with its checkpoints."""
import copy
import math

import pytest
import torch

pytestmark = pytest.mark.timeout(600)

CPU = torch.device("cpu")
U = 2.0 ** -24  # fp32 unit roundoff


def _batches(n, batch, size, classes, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randint(0, 256, (batch, size, size, 3), dtype=torch.uint8, generator=g),
             torch.randint(0, classes, (batch,), generator=g)) for _ in range(n)]


def _trainer(model, optim, **kw):
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer
    return NativeTrainer(model, 4, (32, 32), CPU, optim=optim, use_graphs=False, **kw)


def _bn_pairs(tr, ema_bn_views):
    return [pr for bn, (m, v) in zip(tr.prog.bns, ema_bn_views)
            for pr in ((m, bn.mod.running_mean), (v, bn.mod.running_var))]


def _shadow(tr):
    """An average kept from outside a trainer without one: (flat ema, [(mean, var)] per BN, table)."""
    from dbx_distributed_pytorch_examples_amd.ops import kernels as K
    ema = tr.prog.master.clone()
    views = [(bn.mod.running_mean.clone(), bn.mod.running_var.clone()) for bn in tr.prog.bns]
    pairs = _bn_pairs(tr, views)
    return ema, views, K.pack_ema_desc(pairs, tr.dev), len(pairs), max(bn.C for bn in tr.prog.bns)


def _flat_bn(views):
    return torch.cat([t for mv in views for t in mv])


def _own_bn(tr):
    return torch.cat([t for mv in tr.ema_bn_views for t in mv])


@pytest.mark.parametrize("n", [1, 5, 1023])
def test_reference_ema_update(n):
    """The reference computes fl(e + fl(omd * fl(p - e))): three roundings, one more than the kernel's
    fma. With d = p - e exact in float64: the difference contributes <= u |d| omd, the product
    <= u omd |d| (1 + u), the sum <= u |result|, so
    |got - ref| <= u (|ref| + 2 omd |p - e|) (1 + 2^-20)."""
    from dbx_distributed_pytorch_examples_amd.ops import kernels as K
    from dbx_distributed_pytorch_examples_amd.ops import reference as R
    g = torch.Generator().manual_seed(n)
    p = torch.randn(n, generator=g) * 3 + 0.5
    for decay, via in ((0.9, "scalar"), (0.9999, "scalar"), (0.999, "hyper")):
        e = torch.randn(n, generator=g)
        omd32 = torch.tensor(1.0 - decay, dtype=torch.float32)
        omd = float(omd32)
        ref = e.double() + omd * (p.double() - e.double())
        bound = U * (ref.abs() + 2 * omd * (p.double() - e.double()).abs()) * (1 + 2.0 ** -20)
        got = e.clone()
        if via == "scalar":
            R.ema_update(got, p, one_minus_decay=1.0 - decay)
        else:  # the device scalar wins over the argument
            K.ema_update(got, p, one_minus_decay=0.5, hyper=omd32.reshape(1))
        assert ((got.double() - ref).abs() <= bound).all(), (n, decay)
    with pytest.raises(TypeError):
        K.ema_update(p.double(), p.double(), one_minus_decay=0.1)
    with pytest.raises(ValueError):
        K.ema_update(torch.zeros(n + 1), p, one_minus_decay=0.1)
    with pytest.raises(ValueError):
        K.ema_update(torch.zeros(8)[::2], torch.zeros(4), one_minus_decay=0.1)


def test_reference_ema_update_multi_and_fused():
    from dbx_distributed_pytorch_examples_amd.ops import kernels as K
    g = torch.Generator().manual_seed(0)
    lens = [1, 3, 8, 64]
    dst = [torch.randn(n, generator=g) for n in lens]
    src = [torch.randn(n, generator=g) for n in lens]
    exp = [K.ema_update(d.clone(), s, one_minus_decay=0.01) for d, s in zip(dst, src)]
    desc = K.pack_ema_desc(list(zip(dst, src)), CPU)
    assert desc.shape == (4, 3) and desc.dtype == torch.int64
    K.ema_update_multi(desc, 4, 64, one_minus_decay=0.01)
    assert all(torch.equal(a, b) for a, b in zip(dst, exp))
    with pytest.raises(ValueError):
        K.pack_ema_desc([(dst[0], src[1])], CPU)
    with pytest.raises(TypeError):
        K.pack_ema_desc([(dst[0].double(), src[0].double())], CPU)
    # fused == the plain step followed by ema_update
    n = 37
    p, gr, v, e = (torch.randn(n, generator=g) for _ in range(4))
    p2, v2, e2 = p.clone(), v.clone(), e.clone()
    K.sgd_step(p, gr, v, None, lr=0.1, momentum=0.9, weight_decay=1e-4, ema=e, ema_one_minus_decay=0.01)
    K.sgd_step(p2, gr, v2, None, lr=0.1, momentum=0.9, weight_decay=1e-4)
    K.ema_update(e2, p2, one_minus_decay=0.01)
    assert torch.equal(p, p2) and torch.equal(v, v2) and torch.equal(e, e2)
    m, m2, v, v2 = (torch.zeros(n) for _ in range(4))  # (Adam's second moment is non-negative)
    kw = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, decoupled=True, step=1)
    K.adam_step(p, gr, m, v, None, ema=e, ema_hyper=torch.tensor([0.25]), **kw)
    K.adam_step(p2, gr, m2, v2, None, **kw)
    K.ema_update(e2, p2, one_minus_decay=0.25)
    assert torch.equal(p, p2) and torch.equal(e, e2)
    with pytest.raises(ValueError):
        K.sgd_step(p, gr, v, None, lr=0.1, momentum=0.9, ema=torch.zeros(n + 1))
    with pytest.raises(TypeError):
        K.adam_step(p, gr, m, v, None, ema=torch.zeros(n, dtype=torch.float64), **kw)


def test_ema_decay_at():
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig
    from dbx_distributed_pytorch_examples_amd.models import build_model
    torch.manual_seed(0)
    m = build_model("resnet18", num_classes=10)
    tr = _trainer(copy.deepcopy(m), OptimConfig(lr=0.1), ema_decay=0.999, ema_warmup=True)
    assert tr.ema_decay_at(1) == 2.0 / 11.0 and tr.ema_decay_at(2) == 3.0 / 12.0
    assert tr.ema_decay_at(8990) == 8991.0 / 9000.0 and tr.ema_decay_at(8991) == 0.999
    assert tr.ema_decay_at(10 ** 6) == 0.999
    flat = _trainer(copy.deepcopy(m), OptimConfig(lr=0.1), ema_decay=0.9)
    assert flat.ema_decay_at(1) == flat.ema_decay_at(1000) == 0.9
    assert flat.ema.shape == (flat.prog.n_params,) and torch.equal(flat.ema, flat.prog.master)
    assert flat.ema.data_ptr() != flat.prog.master.data_ptr()
    off = _trainer(copy.deepcopy(m), OptimConfig(lr=0.1))
    assert off.ema is None and off.ema_bn is None
    for bad in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError):
            _trainer(copy.deepcopy(m), OptimConfig(lr=0.1), ema_decay=bad)
    for stage in (1, 2):
        with pytest.raises(ValueError, match="zero_stage"):
            NativeTrainer(copy.deepcopy(m), 4, (32, 32), CPU, optim=OptimConfig(lr=0.1), use_graphs=False,
                          zero_stage=stage, ema_decay=0.9)
    with pytest.raises(ValueError):
        off.evaluate_batch(*_batches(1, 4, 32, 10)[0], use_ema=True)
    with pytest.raises(ValueError):
        off.ema_state_dict()


@pytest.mark.parametrize("optim,clip", [("sgd", 0.0), ("adamw", 0.0), ("lars", 0.5)])
def test_trainer_twins(optim, clip):
    """A (fused average) against B (no average; the test applies ema_update / ema_update_multi after
    every step with omd from ema_decay_at): the same reference arithmetic, so bit-identical."""
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import OptimConfig
    from dbx_distributed_pytorch_examples_amd.models import build_model
    from dbx_distributed_pytorch_examples_amd.ops import kernels as K
    torch.manual_seed(0)
    m1 = build_model("resnet18", num_classes=10)
    m2 = copy.deepcopy(m1)
    lr0 = {"adamw": 1e-3, "sgd": 0.05, "lars": 2.0}[optim]
    oc = OptimConfig(name=optim, lr=lr0, grad_clip=clip, weight_decay=1e-4)
    a = _trainer(m1, copy.copy(oc), ema_decay=0.999, ema_warmup=True)
    b = _trainer(m2, copy.copy(oc))
    ema, views, desc, nt, mx = _shadow(b)
    for i, (x, y) in enumerate(_batches(3, 4, 32, 10, seed=3)):
        for t in (a, b):
            t.set_lr(lr0 * 0.8 ** i)
            t.step(x, y)
        omd = 1.0 - a.ema_decay_at(b.step_count)
        K.ema_update(ema, b.prog.master, one_minus_decay=omd)
        K.ema_update_multi(desc, nt, mx, one_minus_decay=omd)
        assert torch.equal(a.prog.master, b.prog.master) and torch.equal(a.mom, b.mom), i
        assert torch.equal(a.ema, ema), i
        assert torch.equal(_own_bn(a), _flat_bn(views)), i
    assert not torch.equal(a.ema, a.prog.master)
    assert a.hyper.numel() == 4  # the schedule has a device scalar of its own
    # the state dict: the model's keys and shapes, averaged values, counters copied
    sd, msd = a.ema_state_dict(), m1.state_dict()
    assert list(sd) == list(msd) and all(sd[k].shape == msd[k].shape and sd[k].dtype == msd[k].dtype for k in sd)
    assert torch.equal(sd["bn1.num_batches_tracked"], msd["bn1.num_batches_tracked"])
    assert not torch.equal(sd["conv1.weight"], msd["conv1.weight"])
    before = (a.ema.clone(), a.ema_bn.clone())
    a.ema.zero_()
    a.ema_bn.zero_()
    a.load_ema_state_dict(sd)
    assert torch.equal(a.ema, before[0]) and torch.equal(a.ema_bn, before[1])
    # evaluation from the average == a fresh trainer built on the averaged model; nothing is left behind
    x, y = _batches(1, 4, 32, 10, seed=9)[0]
    fresh_model = build_model("resnet18", num_classes=10)
    fresh_model.load_state_dict(sd)
    fresh = _trainer(fresh_model, copy.copy(oc))
    le = a.evaluate_batch(x, y, use_ema=True).clone()  # (the logits live in a static buffer)
    assert torch.equal(le, a.evaluate_batch(x, y))  # None: the average when enabled
    assert torch.equal(le, fresh.evaluate_batch(x, y))
    lraw = a.evaluate_batch(x, y, use_ema=False).clone()
    assert torch.equal(lraw, b.evaluate_batch(x, y)) and not torch.equal(lraw, le)
    for t in (a, b):
        t.step(x, y)
    assert torch.equal(a.prog.master, b.prog.master)


def test_boundary_only_updates():
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import OptimConfig
    from dbx_distributed_pytorch_examples_amd.models import build_model
    from dbx_distributed_pytorch_examples_amd.ops import kernels as K
    torch.manual_seed(0)
    m1 = build_model("resnet18", num_classes=10)
    m2 = copy.deepcopy(m1)
    oc = OptimConfig(lr=0.05, weight_decay=1e-4)
    k = 3
    a = _trainer(m1, copy.copy(oc), grad_accum=k, ema_decay=0.9, ema_warmup=True)
    b = _trainer(m2, copy.copy(oc), grad_accum=k)
    ema, views, desc, nt, mx = _shadow(b)
    for i, (x, y) in enumerate(_batches(2 * k, 4, 32, 10, seed=4)):
        prev, prev_bn = a.ema.clone(), a.ema_bn.clone()
        a.step(x, y)
        b.step(x, y)
        if (i + 1) % k:
            assert torch.equal(a.ema, prev) and torch.equal(a.ema_bn, prev_bn), i
            continue
        omd = 1.0 - a.ema_decay_at(b.step_count)
        K.ema_update(ema, b.prog.master, one_minus_decay=omd)
        K.ema_update_multi(desc, nt, mx, one_minus_decay=omd)
        assert torch.equal(a.ema, ema) and not torch.equal(a.ema, prev), i
        assert torch.equal(_own_bn(a), _flat_bn(views)), i
    assert a.step_count == 2


def _cfg(tmp_path, **kw):
    from dbx_distributed_pytorch_examples_amd.config import TrainConfig
    cfg = TrainConfig(model="resnet18", num_classes=10, batch_size=4, epochs=1, log_every=0, engine="native",
                      graphs=False, checkpoint_dir=str(tmp_path / "ck"), **kw)
    cfg.data.image_size = 32
    cfg.data.num_workers = 1
    cfg.optim.lr = 0.02
    return cfg


def test_train_checkpoint_round_trip(tmp_path, monkeypatch, capsys):
    monkeypatch.setenv("DBX_MLRUNS", str(tmp_path / "mlruns"))
    monkeypatch.setenv("DBX_FORCE_CPU", "1")
    from dbx_distributed_pytorch_examples_amd.config import TrainConfig, load_config
    from dbx_distributed_pytorch_examples_amd.data.datasets import SyntheticImages
    from dbx_distributed_pytorch_examples_amd.models import build_model
    from dbx_distributed_pytorch_examples_amd.train.engine import train
    from dbx_distributed_pytorch_examples_amd.utils import checkpoint as ckpt
    assert (TrainConfig().ema_decay, TrainConfig().ema_warmup, TrainConfig().ema_eval) == (0.0, False, True)
    cfg0 = load_config(None, ["ema_decay=0.5", "ema_warmup=true", "ema_eval=false"])
    assert (cfg0.ema_decay, cfg0.ema_warmup, cfg0.ema_eval) == (0.5, True, False)
    tr_ds, ev_ds = SyntheticImages(8, 32, 3, 10, seed=1), SyntheticImages(4, 32, 3, 10, seed=2)
    res = train(_cfg(tmp_path, ema_decay=0.9), train_dataset=tr_ds, eval_dataset=ev_ds, log_mlflow=False)
    assert res.engine == "native" and res.steps == 2
    assert "val_accuracy" in res.history[-1] and math.isfinite(res.history[-1]["val_loss"])
    assert res.ema_state_dict is not None
    build_model("resnet18", num_classes=10).load_state_dict(res.ema_state_dict)
    st = torch.load(ckpt.latest_checkpoint(str(tmp_path / "ck")), map_location="cpu", weights_only=True)
    saved, saved_bn = st["trainer"]["ema"], st["trainer"]["ema_bn"]
    assert not torch.equal(saved, torch.zeros_like(saved))
    # resume: the average is back, bit for bit, before the next step runs
    from dbx_distributed_pytorch_examples_amd.train import engine as E
    seen = {}
    orig = E._restore_trainer_state

    def spy(runner, state):
        orig(runner, state)
        seen["ema"], seen["ema_bn"] = runner.tr.ema.clone(), runner.tr.ema_bn.clone()
        seen["steps"] = runner.tr.step_count

    monkeypatch.setattr(E, "_restore_trainer_state", spy)
    cfg = _cfg(tmp_path, ema_decay=0.9, resume="latest")
    cfg.epochs = 2
    r1 = train(cfg, train_dataset=tr_ds, log_mlflow=False)
    assert r1.resumed_epoch == 1 and r1.steps == 4 and seen["steps"] == 2
    assert torch.equal(seen["ema"], saved) and torch.equal(seen["ema_bn"], saved_bn)
    # a checkpoint written without the average: warning + re-seed from the loaded parameters
    path = ckpt.latest_checkpoint(str(tmp_path / "ck"))
    old = torch.load(path, map_location="cpu", weights_only=True)
    del old["trainer"]["ema"], old["trainer"]["ema_bn"]
    torch.save(old, path)
    capsys.readouterr()
    cfg = _cfg(tmp_path, ema_decay=0.9, resume="latest")
    cfg.epochs = int(old["epoch"])  # complete: no step runs, the trainer stays as restored
    r2 = train(cfg, train_dataset=tr_ds, log_mlflow=False)
    assert "carries no weight EMA" in capsys.readouterr().out
    sd = r2.model.state_dict()
    assert all(torch.equal(r2.ema_state_dict[k], sd[k].cpu()) for k in sd)


def test_restore_brings_the_average_back():
    from types import SimpleNamespace

    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import OptimConfig
    from dbx_distributed_pytorch_examples_amd.models import build_model
    from dbx_distributed_pytorch_examples_amd.train.engine import _restore_trainer_state, _trainer_state
    torch.manual_seed(0)
    m = build_model("resnet18", num_classes=10)
    a = _trainer(m, OptimConfig(lr=0.05), ema_decay=0.9)
    for x, y in _batches(2, 4, 32, 10):
        a.step(x, y)
    st = _trainer_state(SimpleNamespace(tr=a))
    assert set(st) == {"kind", "mom", "step_count", "ema", "ema_bn"}
    b = _trainer(build_model("resnet18", num_classes=10), OptimConfig(lr=0.05), ema_decay=0.9)
    b.prog.model.load_state_dict(m.state_dict())
    b.params_changed()
    assert torch.equal(b.ema, b.prog.master) and torch.equal(b.prog.master, a.prog.master)
    _restore_trainer_state(SimpleNamespace(tr=b), st)
    assert torch.equal(b.ema, a.ema) and torch.equal(b.ema_bn, a.ema_bn) and b.step_count == 2
    x, y = _batches(1, 4, 32, 10, seed=7)[0]
    a.step(x, y)
    b.step(x, y)
    assert torch.equal(b.ema, a.ema) and torch.equal(b.prog.master, a.prog.master)


def test_train_refuses_ema_without_the_native_step(tmp_path, monkeypatch):
    monkeypatch.setenv("DBX_MLRUNS", str(tmp_path / "mlruns"))
    monkeypatch.setenv("DBX_FORCE_CPU", "1")
    from dbx_distributed_pytorch_examples_amd.data.datasets import SyntheticImages
    from dbx_distributed_pytorch_examples_amd.train.engine import train
    ds = SyntheticImages(8, 32, 3, 10, seed=1)
    cfg = _cfg(tmp_path, ema_decay=0.9)
    cfg.engine = "autograd"
    with pytest.raises(ValueError, match="ema_decay"):
        train(cfg, train_dataset=ds, log_mlflow=False)
    cfg = _cfg(tmp_path, ema_decay=1.0)
    with pytest.raises(ValueError, match="ema_decay"):
        train(cfg, train_dataset=ds, log_mlflow=False)
