"""Weight EMA in the native training step on the GPU: the standalone kernel per element against a
float64 computation with a derived bound, the table-driven launch, fused == unfused bit for bit,
trainers with the fused average against twins averaged from outside (graphs on, a decay schedule),
gradient accumulation, the optimizer inside the backward, per-segment graphs, evaluation from the
average, and train() with checkpoints."""
import copy
import math

import pytest
import torch
import torch.distributed as dist

pytestmark = pytest.mark.gpu

dev = torch.device("cuda")
U = 2.0 ** -24  # fp32 unit roundoff

# (dst offset, src offset) in elements inside 16-byte aligned buffers, as in test_grad_accum_gpu.py:
# both aligned (vector path, also at a non-zero offset), dst / src / both misaligned (scalar path)
_OFFSETS = [(0, 0), (4, 4), (1, 0), (0, 1), (2, 0), (0, 2), (1, 1), (2, 2), (1, 2)]


@pytest.fixture
def world1(tmp_path):
    if not dist.is_initialized():
        dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    yield
    dist.destroy_process_group()


def _batches(n, batch, size, classes, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randint(0, 256, (batch, size, size, 3), dtype=torch.uint8, generator=g).to(dev),
             torch.randint(0, classes, (batch,), generator=g).to(dev)) for _ in range(n)]


def _normal(n, g, scale=1.0):
    """fp32 values in the normal range: magnitudes in [2^-6, 2^6) * scale, random signs."""
    mag = torch.exp2(torch.rand(n, generator=g) * 12 - 6) * scale
    sign = torch.randint(0, 2, (n,), generator=g).float() * 2 - 1
    return (mag * sign).float()


def _shadow(tr):
    """An average kept from outside a trainer that has none: flat ema, [(mean, var)] per BN, its table."""
    from dbx_distributed_pytorch_examples_amd.ops import kernels as K
    ema = tr.prog.master.clone()
    views = [(bn.mod.running_mean.clone(), bn.mod.running_var.clone()) for bn in tr.prog.bns]
    pairs = [pr for bn, (m, v) in zip(tr.prog.bns, views)
             for pr in ((m, bn.mod.running_mean), (v, bn.mod.running_var))]
    return ema, views, K.pack_ema_desc(pairs, dev), len(pairs), max(bn.C for bn in tr.prog.bns)


def _flat(views):
    return torch.cat([t for mv in views for t in mv])


def _advance(tr, omd, ema, desc, nt, mx):
    from dbx_distributed_pytorch_examples_amd.ops import kernels as K
    K.ema_update(ema, tr.prog.master, one_minus_decay=omd)
    K.ema_update_multi(desc, nt, mx, one_minus_decay=omd)


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4096 + 7, (1 << 20) + 1])
def test_ema_update_per_element(n):
    """got = fma(omd, fl(p - e), e): one rounding of the difference (relative u, carried through the
    product: u omd |p - e|) and one of the fma (u |result|), so against float64 from the same fp32
    inputs  |got - ref| <= u (|ref| + omd |p - e|) (1 + 2^-20).
    Largest err / bound measured on an MI355X: 0.9992 (n = 2^20 + 1; 0.67-0.99 for the smaller sizes)."""
    from dbx_distributed_pytorch_examples_amd.ops import kernels as K
    g = torch.Generator().manual_seed(n)
    pad = 8
    src_buf = _normal(n + 2 * pad, g).to(dev)
    dst_init = _normal(n + 2 * pad, g).to(dev)
    worst = 0.0
    for decay in (0.9, 0.9999):
        omd32 = torch.tensor([1.0 - decay], dtype=torch.float32)  # double on the host, rounded once
        omd = float(omd32)
        hyper = omd32.to(dev)
        for do, so in _OFFSETS:
            src = src_buf[so:so + n]
            for mode in ("scalar", "pointer"):
                dst_buf = dst_init.clone()
                dst = dst_buf[do:do + n]
                assert (dst.data_ptr() % 16 == 0) == (do % 4 == 0) and (src.data_ptr() % 16 == 0) == (so % 4 == 0)
                if mode == "scalar":
                    K.ema_update(dst, src, one_minus_decay=1.0 - decay)
                else:  # the device scalar wins over the argument
                    K.ema_update(dst, src, one_minus_decay=0.5, hyper=hyper)
                e64, p64 = dst_init[do:do + n].double(), src.double()
                ref = e64 + omd * (p64 - e64)
                bound = U * (ref.abs() + omd * (p64 - e64).abs()) * (1 + 2.0 ** -20)
                err = (dst.double() - ref).abs()
                worst = max(worst, (err / bound).max().item())
                assert (err <= bound).all(), (n, decay, do, so, mode, (err / bound).max().item())
                assert torch.equal(dst_buf[:do], dst_init[:do]) and torch.equal(dst_buf[do + n:], dst_init[do + n:]), \
                    (n, do, so, mode)
    print(f"ema_update n={n}: largest err / bound = {worst:.4f}")
    with pytest.raises(TypeError):
        K.ema_update(dst_init.double(), src_buf.double(), one_minus_decay=0.1)
    with pytest.raises(ValueError):
        K.ema_update(dst_init, src_buf[:-1], one_minus_decay=0.1)
    with pytest.raises(ValueError):
        K.ema_update(torch.zeros(16, device=dev)[::2], torch.zeros(8, device=dev), one_minus_decay=0.1)
    with pytest.raises(TypeError):
        K.ema_update(dst_init, src_buf, hyper=torch.zeros(1, device=dev, dtype=torch.float64))


def test_ema_update_multi():
    """One launch over a table == one ema_update per entry, bit for bit; two entries sit at addresses
    that are only 4-byte aligned (scalar path); the elements between the entries stay as they were."""
    from dbx_distributed_pytorch_examples_amd.ops import kernels as K
    g = torch.Generator().manual_seed(0)
    lens = [1, 3, 8, 64, 72, 2048]
    shift = [0, 0, 1, 0, 2, 0]  # entries 2 and 4: destination (and source) off the 16-byte grid
    offs, o = [], 0
    for n, s in zip(lens, shift):
        offs.append(o + s)
        o += (n + s + 3) // 4 * 4 + 8  # at least 8 guard elements after every entry
    dbuf0, sbuf = _normal(o, g).to(dev), _normal(o, g).to(dev)
    hyper = torch.tensor([0.125], device=dev)
    for omd, hy in ((0.01, None), (0.5, hyper)):
        dbuf, dref = dbuf0.clone(), dbuf0.clone()
        dst = [dbuf[a:a + n] for a, n in zip(offs, lens)]
        src = [sbuf[a:a + n] for a, n in zip(offs, lens)]
        assert [d.data_ptr() % 16 != 0 for d in dst] == [s != 0 for s in shift]
        desc = K.pack_ema_desc(list(zip(dst, src)), dev)
        assert desc.shape == (len(lens), 3) and desc.dtype == torch.int64 and desc.is_cuda
        K.ema_update_multi(desc, len(lens), max(lens), one_minus_decay=omd, hyper=hy)
        for a, n in zip(offs, lens):
            K.ema_update(dref[a:a + n], sbuf[a:a + n], one_minus_decay=omd, hyper=hy)
        assert torch.equal(dbuf, dref)
        keep = torch.ones(o, dtype=torch.bool, device=dev)
        for a, n in zip(offs, lens):
            keep[a:a + n] = False
            assert not torch.equal(dbuf[a:a + n], dbuf0[a:a + n])
        assert torch.equal(dbuf[keep], dbuf0[keep])
    with pytest.raises(ValueError):
        K.ema_update_multi(desc, len(lens) + 1, max(lens), one_minus_decay=0.1)
    with pytest.raises(TypeError):
        K.ema_update_multi(desc.int(), len(lens), max(lens), one_minus_decay=0.1)
    with pytest.raises(ValueError):
        K.pack_ema_desc([(dbuf[:4], sbuf[:5])], dev)
    with pytest.raises(TypeError):
        K.pack_ema_desc([(dbuf[:4].double(), sbuf[:4].double())], dev)


@pytest.mark.parametrize("n", [5, 1023, 4096 + 7])
def test_fused_equals_unfused(n):
    """sgd_step / adam_step with ema= against the plain step followed by ema_update: p, the optimizer
    state, the average and the bf16 copy bit for bit, three calls in a row so the average compounds."""
    from dbx_distributed_pytorch_examples_amd.ops import kernels as K
    g = torch.Generator().manual_seed(n)
    p0, e0 = torch.randn(n, generator=g).to(dev), torch.randn(n, generator=g).to(dev)
    grads = [torch.randn(n, generator=g).to(dev) for _ in range(3)]
    gsp = torch.tensor([0.37], device=dev)
    omd_t = torch.tensor([1.0 - 0.999], device=dev)
    cases = [(mom, nest, p16, sp) for mom in (0.0, 0.9) for nest in ((False, True) if mom else (False,))
             for p16 in (False, True) for sp in (False, True)]
    for mom, nest, use16, use_sp in cases:
        st = [[p0.clone(), torch.zeros(n, device=dev), e0.clone(),
               torch.zeros(n, device=dev, dtype=torch.bfloat16) if use16 else None] for _ in range(2)]
        for i, gr in enumerate(grads):
            kw = dict(lr=0.1 * 0.5 ** i, momentum=mom, weight_decay=1e-4, nesterov=nest,
                      grad_scale_ptr=gsp if use_sp else None, grad_scale=0.5)
            hy = omd_t if i == 1 else None  # the pointer (0.001) wins over the scalar there
            (p, v, e, p16), (q, w, f, q16) = st
            K.sgd_step(p, gr, v, p16, ema=e, ema_hyper=hy, ema_one_minus_decay=0.01, **kw)
            K.sgd_step(q, gr, w, q16, **kw)
            K.ema_update(f, q, one_minus_decay=0.01, hyper=hy)
            assert torch.equal(p, q) and torch.equal(v, w) and torch.equal(e, f), (n, mom, nest, use16, use_sp, i)
            assert p16 is None or torch.equal(p16, q16)
        assert not torch.equal(st[0][2], e0)
    for decoupled in (False, True):
        for use16 in (False, True):
            st = [[p0.clone(), torch.zeros(n, device=dev), torch.zeros(n, device=dev), e0.clone(),
                   torch.zeros(n, device=dev, dtype=torch.bfloat16) if use16 else None] for _ in range(2)]
            for i, gr in enumerate(grads):
                kw = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, decoupled=decoupled,
                          step=i + 1, grad_scale_ptr=gsp if i else None, grad_scale=0.5)
                hy = omd_t if i == 1 else None
                (p, m, v, e, p16), (q, m2, w, f, q16) = st
                K.adam_step(p, gr, m, v, p16, ema=e, ema_hyper=hy, ema_one_minus_decay=0.01, **kw)
                K.adam_step(q, gr, m2, w, q16, **kw)
                K.ema_update(f, q, one_minus_decay=0.01, hyper=hy)
                assert torch.equal(p, q) and torch.equal(m, m2) and torch.equal(v, w) and torch.equal(e, f), \
                    (n, decoupled, use16, i)
                assert p16 is None or torch.equal(p16, q16)
            assert not torch.equal(st[0][3], e0)
    with pytest.raises(ValueError):
        K.sgd_step(p0.clone(), grads[0], torch.zeros(n, device=dev), None, lr=0.1, momentum=0.9,
                   ema=torch.zeros(n + 1, device=dev))
    with pytest.raises(TypeError):
        K.sgd_step(p0.clone(), grads[0], torch.zeros(n, device=dev), None, lr=0.1, momentum=0.9,
                   ema=torch.zeros(n, device=dev, dtype=torch.float64))
    with pytest.raises(ValueError):
        K.sgd_step(p0.clone(), grads[0], torch.zeros(n, device=dev), None, lr=0.1, momentum=0.9,
                   ema=torch.zeros(2 * n, device=dev)[::2])


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("optim,clip", [("sgd", 0.0), ("adamw", 0.0), ("lars", 0.5)])
@pytest.mark.parametrize("arch,size,batch", [("resnet18", 32, 16), ("resnet50", 64, 8)])
def test_trainer_twins(arch, size, batch, optim, clip):
    """A: ema_decay=0.999 with warm-up, graphs on (two eager steps, one capture, three replays; the lr
    and the decay change every step, so a replay provably reads its own 1 - d_t). B: no average; the
    test averages B's master and running statistics itself after every step."""
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig
    from dbx_distributed_pytorch_examples_amd.models import build_model
    torch.manual_seed(0)
    m1 = build_model(arch, num_classes=10)
    m2 = copy.deepcopy(m1)
    lr0 = {"adamw": 1e-3, "sgd": 0.05, "lars": 2.0}[optim]

    def mk(m, **kw):
        oc = OptimConfig(name=optim, lr=lr0, grad_clip=clip, weight_decay=1e-4)
        return NativeTrainer(m, batch, (size, size), dev, optim=oc, **kw)

    a, b = mk(m1, ema_decay=0.999, ema_warmup=True), mk(m2)
    assert b.ema is None and b.ema_bn is None
    assert torch.equal(a.ema, a.prog.master) and a.hyper.numel() == 4
    ema, views, desc, nt, mx = _shadow(b)
    for i, (x, y) in enumerate(_batches(6, batch, size, 10, seed=5)):
        for t in (a, b):
            t.set_lr(lr0 * 0.8 ** i)
            t.step(x, y)
        assert a.ema_decay_at(i + 1) == (2.0 + i) / (11.0 + i) and b.step_count == i + 1
        _advance(b, 1.0 - a.ema_decay_at(b.step_count), ema, desc, nt, mx)
        assert torch.equal(a.prog.master, b.prog.master) and torch.equal(a.mom, b.mom), i
        assert a.mom2 is None or torch.equal(a.mom2, b.mom2), i
        assert torch.equal(a.ema, ema), i
        assert torch.equal(_flat(a.ema_bn_views), _flat(views)), i
    assert len(a.graphs) == 1 and len(b.graphs) == 1
    assert not torch.equal(a.ema, a.prog.master)
    assert not torch.equal(_flat(views), _flat([(bn.mod.running_mean, bn.mod.running_var) for bn in b.prog.bns]))


def test_grad_accum_moves_the_average_on_boundaries_only():
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig
    from dbx_distributed_pytorch_examples_amd.models import build_model
    torch.manual_seed(0)
    m1 = build_model("resnet18", num_classes=10)
    m2 = copy.deepcopy(m1)
    mk = lambda m, **kw: NativeTrainer(m, 16, (32, 32), dev, optim=OptimConfig(lr=0.05, weight_decay=1e-4),  # noqa: E731
                                       grad_accum=2, **kw)
    a, b = mk(m1, ema_decay=0.999, ema_warmup=True), mk(m2)
    ema, views, desc, nt, mx = _shadow(b)
    for i, (x, y) in enumerate(_batches(10, 16, 32, 10, seed=6)):
        prev, prev_bn = a.ema.clone(), a.ema_bn.clone()
        for t in (a, b):
            t.set_lr(0.05 * 0.9 ** i)
            t.step(x, y)
        if i % 2 == 0:  # micro-step
            assert torch.equal(a.ema, prev) and torch.equal(a.ema_bn, prev_bn), i
            continue
        _advance(b, 1.0 - a.ema_decay_at(b.step_count), ema, desc, nt, mx)
        assert torch.equal(a.prog.master, b.prog.master), i
        assert torch.equal(a.ema, ema) and not torch.equal(a.ema, prev), i
        assert torch.equal(_flat(a.ema_bn_views), _flat(views)), i
    assert a.step_count == 5 and len(a.graphs) == 1 and len(a.micro_graphs) == 1


@pytest.mark.parametrize("arch,size,batch,optim", [("resnet50", 64, 32, "sgd"), ("resnet18", 32, 64, "sgd"),
                                                   ("resnet50", 64, 32, "adamw")])
def test_optimizer_in_backward(arch, size, batch, optim, engine):
    """The per-segment updates on the side stream carry their slice of the average along."""
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig
    from dbx_distributed_pytorch_examples_amd.models import build_model
    o = OptimConfig(lr=0.05) if optim == "sgd" else OptimConfig(name="adamw", lr=1e-3, weight_decay=0.01)
    torch.manual_seed(0)
    m1 = build_model(arch, num_classes=10)
    m2 = copy.deepcopy(m1)
    engine(overlap_optimizer=-1)
    t1 = NativeTrainer(m1, batch, (size, size), dev, optim=o, ema_decay=0.999, ema_warmup=True)
    engine(overlap_optimizer=0)
    t2 = NativeTrainer(m2, batch, (size, size), dev, optim=o, ema_decay=0.999, ema_warmup=True)
    assert t1.opt_ranges is not None and t2.opt_ranges is None
    for x, y in _batches(6, batch, size, 10, seed=5):
        t1.step(x, y)
        t2.step(x, y)
    torch.cuda.synchronize()
    assert torch.equal(t1.prog.master, t2.prog.master)
    assert torch.equal(t1.ema, t2.ema) and torch.equal(t1.ema_bn, t2.ema_bn)
    assert not torch.equal(t1.ema, t1.prog.master)


def test_per_segment_graphs(world1, engine):
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig
    from dbx_distributed_pytorch_examples_amd.models import build_model
    torch.manual_seed(0)
    m1 = build_model("resnet18", num_classes=10)
    m2 = copy.deepcopy(m1)
    mk = lambda m: NativeTrainer(m, 16, (32, 32), dev, optim=OptimConfig(lr=0.05), ema_decay=0.999,  # noqa: E731
                                 ema_warmup=True)
    engine(segmented_graphs="1", comm="torch")  # c10d collectives between per-segment graph replays
    t1 = mk(m1)
    engine(segmented_graphs=None, comm=None)
    t2 = mk(m2)
    assert t1.segmented and t1.ncomm is None and not t2.segmented
    for x, y in _batches(5, 16, 32, 10, seed=8):
        t1.step(x, y)
        t2.step(x, y)
    torch.cuda.synchronize()
    assert len(t1.graphs) > 1 and len(t2.graphs) == 1
    assert torch.equal(t1.prog.master, t2.prog.master)
    assert torch.equal(t1.ema, t2.ema) and torch.equal(t1.ema_bn, t2.ema_bn)
    assert not torch.equal(t1.ema, t1.prog.master)


def test_evaluation_from_the_average():
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig
    from dbx_distributed_pytorch_examples_amd.models import build_model
    torch.manual_seed(0)
    m1 = build_model("resnet18", num_classes=10)
    m2 = copy.deepcopy(m1)
    mk = lambda m, **kw: NativeTrainer(m, 16, (32, 32), dev, optim=OptimConfig(lr=0.05), **kw)  # noqa: E731
    a, b = mk(m1, ema_decay=0.9), mk(m2, ema_decay=0.9)
    data = _batches(5, 16, 32, 10, seed=2)
    for x, y in data[:3]:
        a.step(x, y)
        b.step(x, y)
    xe, ye = data[4]
    sd, msd = a.ema_state_dict(), m1.state_dict()
    assert list(sd) == list(msd)
    assert all(sd[k].shape == msd[k].shape and sd[k].dtype == msd[k].dtype for k in sd)
    assert torch.equal(sd["bn1.num_batches_tracked"], msd["bn1.num_batches_tracked"])
    assert not torch.equal(sd["layer1.0.conv1.weight"], msd["layer1.0.conv1.weight"])
    assert not torch.equal(sd["bn1.running_var"], msd["bn1.running_var"])
    fresh_model = build_model("resnet18", num_classes=10)
    fresh_model.load_state_dict(sd)
    fresh = mk(fresh_model)
    le = a.evaluate_batch(xe, ye, use_ema=True).clone()  # (the logits live in a static buffer)
    assert torch.equal(le, a.evaluate_batch(xe, ye))  # None: the average when enabled
    assert torch.equal(le, fresh.evaluate_batch(xe, ye, use_ema=False))
    lraw = a.evaluate_batch(xe, ye, use_ema=False).clone()
    assert not torch.equal(lraw, le)
    a.evaluate_batch(xe, ye, use_ema=True)  # between steps 3 and 4; b does not evaluate
    a.step(*data[3])
    b.step(*data[3])
    torch.cuda.synchronize()
    assert torch.equal(a.prog.master, b.prog.master) and torch.equal(a.ema, b.ema)
    assert torch.equal(a.ema_bn, b.ema_bn)
    # the inverse
    keep = (a.ema.clone(), a.ema_bn.clone())
    sd = a.ema_state_dict()
    a.ema.zero_()
    a.ema_bn.zero_()
    a.load_ema_state_dict(sd)
    assert torch.equal(a.ema, keep[0]) and torch.equal(a.ema_bn, keep[1])
    with pytest.raises(ValueError):
        fresh.evaluate_batch(xe, ye, use_ema=True)


def test_train_end_to_end(tmp_path, monkeypatch):
    monkeypatch.setenv("DBX_MLRUNS", str(tmp_path / "mlruns"))
    from dbx_distributed_pytorch_examples_amd.config import TrainConfig
    from dbx_distributed_pytorch_examples_amd.data.datasets import SyntheticImages
    from dbx_distributed_pytorch_examples_amd.models import build_model
    from dbx_distributed_pytorch_examples_amd.train import engine as E
    from dbx_distributed_pytorch_examples_amd.utils import checkpoint as ckpt

    def cfg_(**kw):
        cfg = TrainConfig(model="resnet18", num_classes=10, batch_size=32, epochs=2, log_every=0, ema_decay=0.9,
                          checkpoint_dir=str(tmp_path / "ck"), **kw)
        cfg.data.image_size = 32
        cfg.optim.lr = 0.02
        return cfg

    tr_ds, ev_ds = SyntheticImages(128, 32, 3, 10, seed=1), SyntheticImages(64, 32, 3, 10, seed=2)
    res = E.train(cfg_(), train_dataset=tr_ds, eval_dataset=ev_ds, log_mlflow=False)
    assert res.engine == "native" and res.steps == 8
    assert all("val_accuracy" in h and math.isfinite(h["val_loss"]) for h in res.history)
    build_model("resnet18", num_classes=10).load_state_dict(res.ema_state_dict)
    msd = res.model.state_dict()
    assert not torch.equal(res.ema_state_dict["fc.weight"], msd["fc.weight"].cpu())
    st = torch.load(ckpt.latest_checkpoint(str(tmp_path / "ck")), map_location="cpu", weights_only=True)
    saved, saved_bn = st["trainer"]["ema"], st["trainer"]["ema_bn"]
    assert saved.abs().sum() > 0
    seen = {}
    orig = E._restore_trainer_state

    def spy(runner, state):  # right after the restore, before the next step runs
        orig(runner, state)
        seen["ema"], seen["ema_bn"] = runner.tr.ema.cpu(), runner.tr.ema_bn.cpu()

    monkeypatch.setattr(E, "_restore_trainer_state", spy)
    cfg = cfg_(resume="latest")
    cfg.epochs = 3
    r2 = E.train(cfg, train_dataset=tr_ds, log_mlflow=False)
    assert r2.resumed_epoch == 2 and r2.steps == 12
    assert torch.equal(seen["ema"], saved) and torch.equal(seen["ema_bn"], saved_bn)
    off = E.train(TrainConfig(model="resnet18", num_classes=10, batch_size=32, max_steps=1, log_every=0,
                              data=cfg.data), train_dataset=tr_ds, log_mlflow=False)
    assert off.ema_state_dict is None
