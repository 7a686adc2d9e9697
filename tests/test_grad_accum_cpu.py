"""Gradient accumulation in the native training step, on the CPU reference ops: the accumulate op,
exact windows for every optimizer family (the divisor k applied once, in fp32, in the optimizer),
engine selection, and two gloo ranks (no collective inside a window, replicas in sync)."""
import copy

import pytest
import torch

from dbx_distributed_pytorch_examples_amd.launch import Launcher

pytestmark = pytest.mark.timeout(600)

CPU = torch.device("cpu")


def _batches(n, batch, size, classes, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randint(0, 256, (batch, size, size, 3), dtype=torch.uint8, generator=g),
             torch.randint(0, classes, (batch,), generator=g)) for _ in range(n)]


def _harvest(model, batch, size, data, dev=CPU):
    """Per-micro-batch gradients at fixed weights: a grad_accum=1 trainer with lr = 0."""
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig
    tr = NativeTrainer(model, batch, (size, size), dev, optim=OptimConfig(lr=0.0, momentum=0.0, weight_decay=0.0),
                       use_graphs=False)
    out = []
    for x, y in data:
        tr.step(x.to(dev), y.to(dev))
        out.append(tr.prog.grad.clone())
    return out


def _window_sum(gs):
    """The kernel's summation order: acc = g1, acc += g2, ..., grad_k += acc."""
    acc = gs[0].clone()
    for g in gs[1:-1]:
        acc = acc + g
    return gs[-1] + acc


def test_reference_grad_accum():
    from dbx_distributed_pytorch_examples_amd.ops import reference as R
    g = torch.Generator().manual_seed(0)
    src = torch.randn(1001, generator=g)
    dst0 = torch.randn(1001, generator=g)
    dst = dst0.clone()
    R.grad_accum(dst, src)
    assert torch.equal(dst, dst0 + src)
    for kw in ({"first": True}, {"flag": torch.tensor([1.0])}):
        dst = torch.full((1001,), float("nan"))
        R.grad_accum(dst, src, **kw)
        assert torch.equal(dst, src), kw
    dst = dst0.clone()
    R.grad_accum(dst, src, first=True, flag=torch.tensor([0.0]))  # the flag overrides ``first``
    assert torch.equal(dst, dst0 + src)
    with pytest.raises(TypeError):
        R.grad_accum(dst, src.double())
    with pytest.raises(ValueError):
        R.grad_accum(dst, src[:-1])


def test_kernels_grad_accum_dispatches_to_reference_on_cpu():
    from dbx_distributed_pytorch_examples_amd.ops import kernels as K
    src, dst = torch.arange(5.0), torch.ones(5)
    K.grad_accum(dst, src)
    assert torch.equal(dst, torch.arange(5.0) + 1)


def test_exact_window_sgd():
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig
    from dbx_distributed_pytorch_examples_amd.models import build_model
    from dbx_distributed_pytorch_examples_amd.ops import kernels as K
    torch.manual_seed(0)
    model = build_model("resnet18", num_classes=10)
    twin = copy.deepcopy(model)
    k, batch, size = 3, 8, 32
    data = _batches(k, batch, size, 10)
    o = OptimConfig(lr=0.05, momentum=0.9, weight_decay=5e-4)
    tr = NativeTrainer(model, batch, (size, size), CPU, optim=o, use_graphs=False, grad_accum=k)
    assert tr.grad_accum == k and tr.micro == 0 and not tr.at_boundary
    init = tr.prog.master.clone()
    gs = _harvest(twin, batch, size, data)
    for i, (x, y) in enumerate(data):
        tr.step(x, y)
        if i < k - 1:
            assert torch.equal(tr.prog.master, init), i  # no update inside the window
            assert tr.step_count == 0 and tr.micro == i + 1
            assert tr.at_boundary == (i == k - 2)
    assert tr.step_count == 1 and tr.micro == 0
    gsum = _window_sum(gs)
    assert torch.equal(tr.prog.grad, gsum)  # the unscaled window sum is left in the flat gradient
    exp, mom = init.clone(), torch.zeros_like(init)
    K.sgd_step(exp, gsum, mom, None, lr=o.lr, momentum=o.momentum, dampening=0.0, weight_decay=o.weight_decay,
               nesterov=False, first=False, grad_scale=1.0 / k)
    assert torch.equal(tr.prog.master, exp)
    assert torch.equal(tr.mom, mom)
    # every micro-step counted its batch (BatchNorm's num_batches_tracked, the metrics)
    bn = next(m for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d))
    assert int(bn.num_batches_tracked) == k
    # evaluation between micro-steps leaves the window alone
    tr.step(*data[0])
    acc, micro = tr.acc.clone(), tr.micro
    tr.evaluate_batch(*data[1])
    assert torch.equal(tr.acc, acc) and tr.micro == micro == 1


def test_k1_is_the_plain_step():
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig
    from dbx_distributed_pytorch_examples_amd.models import build_model
    torch.manual_seed(0)
    m1 = build_model("resnet18", num_classes=10)
    m2 = copy.deepcopy(m1)
    o = OptimConfig(lr=0.05, momentum=0.9, weight_decay=5e-4)
    t1 = NativeTrainer(m1, 8, (32, 32), CPU, optim=copy.copy(o), use_graphs=False, grad_accum=1)
    t2 = NativeTrainer(m2, 8, (32, 32), CPU, optim=copy.copy(o), use_graphs=False)
    for x, y in _batches(3, 8, 32, 10):
        t1.step(x, y)
        t2.step(x, y)
    assert torch.equal(t1.prog.master, t2.prog.master)
    assert t1.acc is None and t2.acc is None and t1.micro_phases is None
    assert t1.step_count == t2.step_count == 3
    assert float(t1.hyper[3]) == 0.0
    with pytest.raises(ValueError):
        NativeTrainer(copy.deepcopy(m1), 8, (32, 32), CPU, use_graphs=False, grad_accum=0)


@pytest.mark.parametrize("name,clip,zero", [("adamw", 0.3, 0), ("lars", 0.5, 0), ("sgd", 0.0, 1)])
def test_exact_window_adam_clip_lars_zero(name, clip, zero):
    """The window's update recomputed with the optimizer kernels from harvested micro-batch gradients:
    the divisor k appears once (grad_scale, or the clip's max_norm x k)."""
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig
    from dbx_distributed_pytorch_examples_amd.models import build_model
    from dbx_distributed_pytorch_examples_amd.ops import kernels as K
    torch.manual_seed(0)
    model = build_model("resnet18", num_classes=10)
    twin = copy.deepcopy(model)
    k, batch, size = 3, 8, 32
    data = _batches(k, batch, size, 10, seed=2)
    lr = {"adamw": 1e-3, "lars": 2.0, "sgd": 0.05}[name]
    o = OptimConfig(name=name, lr=lr, momentum=0.9, weight_decay=1e-4, grad_clip=clip)
    tr = NativeTrainer(model, batch, (size, size), CPU, optim=o, use_graphs=False, zero_stage=zero, grad_accum=k)
    init = tr.prog.master.clone()
    gs = _harvest(twin, batch, size, data)
    assert tr.prog.master.numel() == gs[0].numel()  # (same flat layout: world 1)
    for x, y in data:
        assert torch.equal(tr.prog.master, init)
        tr.step(x, y)
    assert tr.step_count == 1
    gsum = _window_sum(gs)
    exp, m, v, work = init.clone(), torch.zeros_like(init), torch.zeros_like(init), torch.zeros(4)
    gsp = K.global_norm_clip_factor(gsum, clip * k, work) if clip else None
    if name == "adamw":
        K.adam_step(exp, gsum, m, v, None, lr=lr, beta1=o.betas[0], beta2=o.betas[1], eps=o.eps,
                    weight_decay=o.weight_decay, decoupled=True, step=1, grad_scale_ptr=gsp, grad_scale=1.0 / k)
    elif name == "lars":
        off, ln, adapt, norms, mx = tr._lars_segments()
        gsum = gsum * gsp
        K.lars_scale(exp, gsum, off, ln, adapt, norms, grad_scale=1.0 / k, eta=o.trust_coefficient,
                     weight_decay=o.weight_decay, max_len=mx)
        K.sgd_step(exp, gsum, m, None, lr=lr, momentum=o.momentum, weight_decay=0.0, first=False, grad_scale=1.0)
    else:
        assert tr.zero is not None and tr.zero.grad_div == k and tr.zero.step_count == 1
        K.sgd_step(exp, gsum, m, None, lr=lr, momentum=o.momentum, weight_decay=o.weight_decay, first=False,
                   grad_scale=1.0 / k)
    assert not torch.equal(exp, init)
    assert torch.equal(tr.prog.master, exp), (tr.prog.master - exp).abs().max()


def test_train_picks_native_engine_with_grad_accum():
    from dbx_distributed_pytorch_examples_amd.config import TrainConfig, from_deepspeed
    from dbx_distributed_pytorch_examples_amd.data.datasets import SyntheticImages
    from dbx_distributed_pytorch_examples_amd.models import FrozenBackboneClassifier, build_model
    from dbx_distributed_pytorch_examples_amd.train.engine import _pick_engine
    ds = SyntheticImages(8, 32, 3, 10)
    cuda = torch.device("cuda")
    cfg = TrainConfig(model="resnet18", num_classes=10, batch_size=4, grad_accum=2)
    model = build_model("resnet18", num_classes=10)
    assert _pick_engine(cfg, model, ds, cuda) == "native"
    assert _pick_engine(cfg, model, ds, CPU) == "autograd"
    cfg4 = from_deepspeed({"gradient_accumulation_steps": 4, "train_micro_batch_size_per_gpu": 4,
                           "zero_optimization": {"stage": 1}}, TrainConfig(model="resnet18", num_classes=10),
                          world_size=1)
    assert cfg4.grad_accum == 4
    assert _pick_engine(cfg4, model, ds, cuda) == "native"
    frozen = FrozenBackboneClassifier("resnet18", num_classes=10)
    assert _pick_engine(TrainConfig(num_classes=10, grad_accum=1), frozen, ds, cuda) == "native"
    assert _pick_engine(TrainConfig(num_classes=10, grad_accum=2), frozen, ds, cuda) == "autograd"


def test_restore_drops_partial_window():
    from types import SimpleNamespace

    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig
    from dbx_distributed_pytorch_examples_amd.models import build_model
    from dbx_distributed_pytorch_examples_amd.train.engine import _restore_trainer_state, _trainer_state
    torch.manual_seed(0)
    tr = NativeTrainer(build_model("resnet18", num_classes=10), 4, (32, 32), CPU, optim=OptimConfig(lr=0.05),
                       use_graphs=False, grad_accum=2)
    tr.step(*_batches(1, 4, 32, 10)[0])
    assert tr.micro == 1
    st = _trainer_state(SimpleNamespace(tr=tr))
    assert set(st) == {"kind", "mom", "step_count"}  # no accumulator in a checkpoint
    _restore_trainer_state(SimpleNamespace(tr=tr), st)
    assert tr.micro == 0 and tr.step_count == 0


# ---------------------------------------------------------------------------------------------
def _two_rank_windows():
    import torch.distributed as dist

    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig
    from dbx_distributed_pytorch_examples_amd.models import build_model
    from dbx_distributed_pytorch_examples_amd.parallel import dist as ddist
    ddist.init_distributed(device="cpu")
    rank = ddist.get_rank()
    out = {}
    for case, seed in (("different", 10 + rank), ("identical", 10)):
        torch.manual_seed(0)
        tr = NativeTrainer(build_model("resnet18", num_classes=4), 4, (32, 32), CPU,
                           optim=OptimConfig(lr=0.05, momentum=0.9, weight_decay=5e-4), use_graphs=False,
                           bucket_cap_mb=1.0, grad_accum=2)
        posts = {"micro": 0, "boundary": 0}
        reduces = {"micro": 0, "boundary": 0}
        kind = ["micro"]
        inner_post, inner_ar = tr._post, dist.all_reduce

        def post(p, inner_post=inner_post, posts=posts, kind=kind):
            posts[kind[0]] += 1
            return inner_post(p)

        def all_reduce(*a, inner_ar=inner_ar, reduces=reduces, kind=kind, **kw):
            reduces[kind[0]] += 1
            return inner_ar(*a, **kw)

        tr._post, dist.all_reduce = post, all_reduce
        try:
            for x, y in _batches(6, 4, 32, 4, seed=seed):  # 3 windows of 2
                kind[0] = "boundary" if tr.at_boundary else "micro"
                tr.step(x, y)
        finally:
            dist.all_reduce = inner_ar
        masters = [torch.empty_like(tr.prog.master) for _ in range(2)]
        dist.all_gather(masters, tr.prog.master)
        out[case] = {"in_sync": torch.equal(masters[0], masters[1]), "posts": posts, "reduces": reduces,
                     "master": tr.prog.master.clone(), "steps": tr.step_count}
    ddist.destroy()
    return out


def test_two_gloo_ranks():
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig
    from dbx_distributed_pytorch_examples_amd.models import build_model
    out = Launcher(2, use_gpu=False).run(_two_rank_windows)
    for case in ("different", "identical"):
        r = out[case]
        assert r["in_sync"], case                      # (a) replicas bit-identical after 3 windows
        assert r["steps"] == 3
        assert r["posts"]["micro"] == 0 and r["reduces"]["micro"] == 0, r  # (b) no collective in a micro-step
        assert r["posts"]["boundary"] > 0 and r["reduces"]["boundary"] > 0, r
    # (c) identical data on both ranks: the sum and the divisor both double, exactly
    torch.manual_seed(0)
    tr = NativeTrainer(build_model("resnet18", num_classes=4), 4, (32, 32), CPU,
                       optim=OptimConfig(lr=0.05, momentum=0.9, weight_decay=5e-4), use_graphs=False, grad_accum=2)
    for x, y in _batches(6, 4, 32, 4, seed=10):
        tr.step(x, y)
    assert torch.equal(out["identical"]["master"], tr.prog.master)
    assert not torch.equal(out["different"]["master"], tr.prog.master)
