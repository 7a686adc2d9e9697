"""Gradient accumulation in the native training step on the GPU: the accumulate kernel against torch
(bitwise, aligned and misaligned slices), exact windows, the two captured step kinds against the
eager step, accumulated gradients against fp32 autograd, the fold's place in front of the captured
collective, and train() end to end."""
import copy
import math

import pytest
import torch
import torch.distributed as dist
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

dev = torch.device("cuda")


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


def _cos(a, b):
    a = a.float().flatten()
    b = b.float().flatten()
    return (a @ b / (a.norm() * b.norm() + 1e-20)).item()


# (dst offset, src offset) in elements inside 16-byte aligned buffers: both aligned (vector path, also
# at a non-zero offset), dst / src / both misaligned (scalar path)
_OFFSETS = [(0, 0), (4, 4), (1, 0), (0, 1), (2, 0), (0, 2), (1, 1), (2, 2), (1, 2)]


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4096 + 7, (1 << 20) + 1])
def test_grad_accum_kernel_matches_torch(n):
    from dbx_distributed_pytorch_examples_amd.ops import kernels as K
    g = torch.Generator().manual_seed(n)
    pad = 8
    src_buf = torch.randn(n + 2 * pad, generator=g).to(dev)
    dst_init = torch.randn(n + 2 * pad, generator=g).to(dev)
    flags = {0: torch.zeros(1, device=dev), 1: torch.ones(1, device=dev)}
    for do, so in _OFFSETS:
        src = src_buf[so:so + n]
        for mode in ("add", "first", "flag0", "flag1"):
            first = mode in ("first", "flag1")
            dst_buf = torch.full_like(dst_init, float("nan")) if first else dst_init.clone()
            guard = torch.randn(2 * pad, generator=g).to(dev)  # the elements around the slice
            dst_buf[:do].copy_(guard[:do])
            dst_buf[do + n:].copy_(guard[:dst_buf.numel() - do - n])
            before = dst_buf.clone()
            dst = dst_buf[do:do + n]
            assert (dst.data_ptr() % 16 == 0) == (do % 4 == 0) and (src.data_ptr() % 16 == 0) == (so % 4 == 0)
            if mode == "add":
                K.grad_accum(dst, src)
            elif mode == "first":
                K.grad_accum(dst, src, first=True)
            else:  # the device flag decides, whatever ``first`` says
                K.grad_accum(dst, src, first=(mode == "flag0"), flag=flags[int(mode[-1])])
            exp = src if first else before[do:do + n] + src
            assert torch.equal(dst, exp), (n, do, so, mode)
            assert torch.equal(dst_buf[:do], before[:do]) and torch.equal(dst_buf[do + n:], before[do + n:]), \
                (n, do, so, mode)
    with pytest.raises(TypeError):
        K.grad_accum(dst_init.double(), src_buf.double())
    with pytest.raises(ValueError):
        K.grad_accum(dst_init, src_buf[:-1])
    with pytest.raises(ValueError):
        K.grad_accum(dst_init[::2], src_buf[::2])


@pytest.mark.parametrize("arch,size,batch", [("resnet18", 32, 16), ("resnet50", 64, 8)])
def test_exact_window_gpu(arch, size, batch):
    """k = 3, eager: no update inside the window; the boundary applies SGD to g3 + ((g1) + g2) with
    grad_scale = 1/3 -- the micro-batch gradients harvested from a twin trainer with lr = 0."""
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig
    from dbx_distributed_pytorch_examples_amd.models import build_model
    from dbx_distributed_pytorch_examples_amd.ops import kernels as K
    torch.manual_seed(0)
    model = build_model(arch, num_classes=10)
    twin = copy.deepcopy(model)
    k = 3
    data = _batches(k, batch, size, 10)
    o = OptimConfig(lr=0.05, momentum=0.9, weight_decay=5e-4)
    tr = NativeTrainer(model, batch, (size, size), dev, optim=o, use_graphs=False, grad_accum=k)
    init = tr.prog.master.clone()
    th = NativeTrainer(twin, batch, (size, size), dev, optim=OptimConfig(lr=0.0, momentum=0.0, weight_decay=0.0),
                       use_graphs=False)
    gs = []
    for x, y in data:
        th.step(x, y)
        gs.append(th.prog.grad.clone())
    for i, (x, y) in enumerate(data):
        tr.step(x, y)
        if i < k - 1:
            assert torch.equal(tr.prog.master, init), i
    assert tr.step_count == 1 and tr.micro == 0
    gsum = gs[2] + (gs[0] + gs[1])
    assert torch.equal(tr.prog.grad, gsum)
    exp, mom = init.clone(), torch.zeros_like(init)
    K.sgd_step(exp, gsum, mom, None, lr=o.lr, momentum=o.momentum, dampening=0.0, weight_decay=o.weight_decay,
               nesterov=False, first=False, grad_scale=1.0 / k)
    assert torch.equal(tr.prog.master, exp)


@pytest.mark.parametrize("optim,clip,zero", [("sgd", 0.0, 0), ("adamw", 0.3, 1), ("lars", 0.5, 0)])
@pytest.mark.parametrize("arch,size,batch", [("resnet50", 64, 32), ("resnet18", 32, 64)])
def test_graph_matches_eager(arch, size, batch, optim, clip, zero):
    """k = 2, 5 windows: both step kinds warm up twice, are captured in window 3 and replayed after;
    the lr changes every micro-step, so a replayed boundary provably applies its own value."""
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig
    from dbx_distributed_pytorch_examples_amd.models import build_model
    torch.manual_seed(0)
    m1 = build_model(arch, num_classes=10)
    m2 = copy.deepcopy(m1)
    lr0 = {"adamw": 1e-3, "sgd": 0.05, "lars": 2.0}[optim]

    def mk(m, graphs):
        oc = OptimConfig(name=optim, lr=lr0, grad_clip=clip, weight_decay=1e-4)
        return NativeTrainer(m, batch, (size, size), dev, optim=oc, use_graphs=graphs, zero_stage=zero, grad_accum=2)

    t1, t2 = mk(m1, True), mk(m2, False)
    data = _batches(10, batch, size, 10, seed=5)
    for i, (x, y) in enumerate(data):
        lr = lr0 * (0.8 ** i)
        for t in (t1, t2):
            t.set_lr(lr)
            t.step(x, y)
        if i % 2 == 1:  # per window
            m_1, m_2 = t1.read_metrics(), t2.read_metrics()
            assert m_1 == m_2 and math.isfinite(m_1[0]), (i, m_1, m_2)
            assert torch.equal(t1.prog.master, t2.prog.master), i
    assert len(t1.graphs) == 1 and len(t1.micro_graphs) == 1
    assert not t2.graphs and not t2.micro_graphs
    assert t1.step_count == t2.step_count == 5
    if zero:
        assert t1.zero.step_count == t2.zero.step_count == 5
    assert torch.equal(t1.prog.master, t2.prog.master)


@pytest.mark.parametrize("arch,size,batch", [("resnet50", 64, 8), ("resnet18", 32, 16)])
def test_accumulated_grads_match_autograd(arch, size, batch):
    """lr = 0, k = 2: the flat gradient after the boundary step against fp32 autograd with two
    backward passes into the same .grad (the thresholds of test_program_matches_autograd)."""
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig
    from dbx_distributed_pytorch_examples_amd.models import build_model
    torch.manual_seed(0)
    model = build_model(arch, num_classes=100)
    for n_, m_ in model.named_modules():  # damped residual branches: see test_program_matches_autograd
        if n_.endswith("bn3") or (n_.endswith("bn2") and "layer" in n_ and arch != "resnet50"):
            torch.nn.init.constant_(m_.weight, 0.2)
    ref = copy.deepcopy(model).to(dev).train()
    tr = NativeTrainer(model, batch, (size, size), dev, optim=OptimConfig(lr=0.0, momentum=0.0, weight_decay=0.0),
                       use_graphs=False, grad_accum=2)
    p = tr.prog
    for x, y in _batches(2, batch, size, 100):
        tr.step(x, y)
        torch.cuda.synchronize()
        xin = p.x4[..., :3].float().permute(0, 3, 1, 2).contiguous()
        F.cross_entropy(ref(xin), y).backward()
    assert tr.step_count == 1
    named_ref = dict(ref.named_parameters())
    for name, prm in model.named_parameters():
        off = (prm.data_ptr() - p.master.data_ptr()) // 4
        gflat = p.grad[off:off + prm.numel()]
        gn = (gflat.view(prm.shape[0], prm.shape[2], prm.shape[3], prm.shape[1]).permute(0, 3, 1, 2)
              if prm.dim() == 4 else gflat.view(prm.shape))
        c = _cos(gn, named_ref[name].grad)
        assert c > (0.9 if prm.dim() > 1 else 0.75), (name, c)


@pytest.mark.parametrize("arch,hw,batch,layout", [("resnet18", 32, 32, "block"), ("resnet50", 64, 16, "block"),
                                                  ("resnet18", 32, 32, "batch")])
def test_fold_precedes_collective(world1, arch, hw, batch, layout, engine):
    """The one-graph step with comm_loopback=2 (every all-reduce doubles its range, the update halves
    it) against the plain one at k = 2: a fold placed behind the all-reduce gives 2 g_k + acc instead
    of 2 (g_k + acc), and the trajectories part."""
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig
    from dbx_distributed_pytorch_examples_amd.models import build_model
    engine(segmented_graphs="1")
    engine(comm="native")
    if layout == "batch":
        engine(multirank_layout="batch")
        engine(comm_side="1")
        engine(side_defer="1")
        engine(lazy_join="0")
    torch.manual_seed(0)
    m1 = build_model(arch, num_classes=10)
    m2 = copy.deepcopy(m1)
    engine(comm_loopback="2")
    t1 = NativeTrainer(m1, batch, (hw, hw), dev, optim=OptimConfig(lr=0.05), grad_accum=2)
    engine(comm_loopback=None)
    t2 = NativeTrainer(m2, batch, (hw, hw), dev, optim=OptimConfig(lr=0.05), grad_accum=2)
    assert t1.ncomm is not None and t1.loopback == 2 and t2.loopback == 1
    assert t1.block_posts == (layout == "block") and t1.late_posts == (layout == "batch")
    for i, (x, y) in enumerate(_batches(6, batch, hw, 10)):
        t1.step(x, y)
        t2.step(x, y)
        assert t1.read_metrics()[0] == t2.read_metrics()[0], i
    assert len(t1.graphs) == 1 and len(t1.micro_graphs) == 1
    assert t1.step_count == t2.step_count == 3
    assert torch.equal(t1.prog.master, t2.prog.master)


def test_train_entrypoint_grad_accum(tmp_path, monkeypatch):
    monkeypatch.setenv("DBX_MLRUNS", str(tmp_path / "mlruns"))
    from dbx_distributed_pytorch_examples_amd.config import TrainConfig
    from dbx_distributed_pytorch_examples_amd.data.datasets import SyntheticImages
    from dbx_distributed_pytorch_examples_amd.train.engine import train
    cfg = TrainConfig(model="resnet18", num_classes=10, batch_size=32, epochs=2, log_every=0, grad_accum=2)
    cfg.data.image_size = 32
    cfg.optim.lr = 0.02
    seen = {}

    def cb(epoch, rec, runner):
        seen["steps"], seen["k"] = runner.tr.step_count, runner.tr.grad_accum

    res = train(cfg, train_dataset=SyntheticImages(128, 32, 3, 10), callbacks=[cb], log_mlflow=False)
    assert res.engine == "native"
    assert res.steps == 8 and seen == {"steps": 8 // 2, "k": 2}
    assert all(math.isfinite(h["train_loss"]) for h in res.history)
