"""SE-ResNet / SE-ResNeXt through the native program on the GPU: against fp32 autograd with the damping and the criteria
of tests/test_program_gpu.py::test_program_matches_autograd, captured against eager, evaluation, training, options."""
import copy

import pytest
import torch
import torch.nn.functional as F

from dbx_distributed_pytorch_examples_amd.models import Bottleneck, ResNet, SEModule, build_model

pytestmark = pytest.mark.gpu
dev = torch.device("cuda")


def _cos(a, b):
    a, b = a.float().flatten(), b.float().flatten()
    return (a @ b / (a.norm() * b.norm() + 1e-20)).item()


def _model(arch, classes=100):
    torch.manual_seed(0)
    if arch == "seresnet50":
        m = ResNet(Bottleneck, [1, 1, 1, 1], num_classes=classes, se_reduction=16)
    elif arch == "mixed":  # layer1.0 plain, layer1.1 gated, layer2.0 plain: the boundary in both directions
        m = ResNet(Bottleneck, [2, 1, 1, 1], num_classes=classes)
        m.layer1[1].se = SEModule(256, 16)
    else:
        m = build_model(arch, num_classes=classes)
    for n_, m_ in m.named_modules():  # test_program_matches_autograd's damping: last-BN gamma = 0.2
        if n_.endswith("bn3") or (n_.endswith("bn2") and "layer" in n_ and arch == "seresnet18"):
            torch.nn.init.constant_(m_.weight, 0.2)
    return m


def _trainer(model, batch, size, **kw):
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig
    kw.setdefault("optim", OptimConfig(lr=0.0, momentum=0.0, weight_decay=0.0))
    kw.setdefault("use_graphs", False)
    return NativeTrainer(model, batch, (size, size), dev, **kw)


def _batch(batch, size, classes, seed=1):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 256, (batch, size, size, 3), dtype=torch.uint8, generator=g).to(dev),
            torch.randint(0, classes, (batch,), generator=g).to(dev))


@pytest.mark.parametrize("fold", [0, 1 << 40])
@pytest.mark.parametrize("arch,size,batch", [("seresnet50", 64, 8), ("seresnet18", 32, 16), ("mixed", 64, 8)])
def test_se_program_matches_autograd(arch, size, batch, fold, engine):
    engine(fold_min_elems=str(fold))
    model = _model(arch)
    ref = copy.deepcopy(model).to(dev).train()
    tr = _trainer(model, batch, size)
    p = tr.prog
    img, lab = _batch(batch, size, p.num_classes)
    tr.step(img, lab)
    torch.cuda.synchronize()
    loss_native = p.metrics[0].item() / batch
    x = p.x4[..., :3].float().permute(0, 3, 1, 2).contiguous()
    loss = F.cross_entropy(ref(x), lab)
    loss.backward()
    print(arch, fold, "loss", loss_native, loss.item())
    assert abs(loss_native - loss.item()) / loss.item() < 3e-2, (loss_native, loss.item())
    named_ref = dict(ref.named_parameters())
    for name, prm in model.named_parameters():
        off = (prm.data_ptr() - p.master.data_ptr()) // 4
        gflat = p.grad[off:off + prm.numel()]
        gn = (gflat.view(prm.shape[0], prm.shape[2], prm.shape[3], prm.shape[1]).permute(0, 3, 1, 2) if prm.dim() == 4
              else gflat.view(prm.shape))
        c = _cos(gn, named_ref[name].grad)
        if ".se." in name:
            print(name, c)
        assert c > (0.9 if prm.dim() > 1 else 0.75), (name, c)
    for (n1, b1), (n2, b2) in zip(model.named_buffers(), ref.named_buffers()):
        if "running_mean" in n1:
            assert _cos(b1, b2) > 0.99 or b2.abs().max() < 1e-3, n1


def test_captured_step_equals_eager_step():
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import OptimConfig
    opt = OptimConfig(lr=0.05, momentum=0.9, weight_decay=1e-4)
    a = _trainer(_model("seresnet50"), 8, 64, optim=opt, use_graphs=True)
    b = _trainer(_model("seresnet50"), 8, 64, optim=opt, use_graphs=False)
    for i in range(3):
        img, lab = _batch(8, 64, 100, seed=10 + i)
        a.step(img, lab)
        b.step(img, lab)
        torch.cuda.synchronize()
        assert torch.equal(a.prog.grad, b.prog.grad) and torch.equal(a.prog.master, b.prog.master), i


def test_eval_forward_matches_torch_eval():
    model = _model("seresnet50")
    ref = copy.deepcopy(model).to(dev).eval()
    tr = _trainer(model, 8, 64)
    img, lab = _batch(8, 64, 100)
    out = tr.evaluate_batch(img, lab).float()
    x = tr.prog.x4[..., :3].float().permute(0, 3, 1, 2).contiguous()
    with torch.no_grad():
        want = ref(x)
    assert _cos(out, want) > 0.98, _cos(out, want)


@pytest.mark.parametrize("opt,kw", [("sgd", {}), ("lamb", {}), ("sgd", {"ema_decay": 0.9})], ids=["sgd", "lamb", "ema"])
def test_training_runs_and_sgd_learns(opt, kw):
    """20 SGD steps on a learnable synthetic task (the label is the brightest image quadrant) make the loss fall; one
    LAMB step and steps with a weight EMA (and an evaluation from it) run and stay finite."""
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import OptimConfig
    o = OptimConfig(lr=0.05, momentum=0.9) if opt == "sgd" else OptimConfig(name="lamb", lr=1e-3)
    tr = _trainer(_model("seresnet18", classes=4), 16, 32, optim=o, **kw)
    g = torch.Generator().manual_seed(3)
    losses = []
    for _ in range(20 if opt == "sgd" and not kw else 2):
        lab = torch.randint(0, 4, (16,), generator=g)
        img = torch.randint(0, 96, (16, 32, 32, 3), dtype=torch.uint8, generator=g)
        for n, q in enumerate(lab.tolist()):
            img[n, (q // 2) * 16:(q // 2) * 16 + 16, (q % 2) * 16:(q % 2) * 16 + 16] += 128
        tr.step(img.to(dev), lab.to(dev))
        losses.append(tr.read_metrics()[0] / 16)
    assert all(l == l for l in losses) and torch.isfinite(tr.prog.master).all()
    if kw:
        assert torch.isfinite(tr.evaluate_batch(img.to(dev), lab.to(dev), use_ema=True).float()).all()
    if len(losses) == 20:
        print(losses)
        assert sum(losses[-3:]) < 0.7 * sum(losses[:3]), losses


def test_state_dict_round_trip_restores_the_se_parameters():
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import OptimConfig
    a = _trainer(_model("seresnet18", classes=4), 16, 32, optim=OptimConfig(lr=0.1, momentum=0.9))
    img, lab = _batch(16, 32, 4)
    a.step(img, lab)
    torch.cuda.synchronize()
    sd = {k: v.detach().cpu().clone() for k, v in a.prog.model.state_dict().items()}
    fresh = _model("seresnet18", classes=4)
    assert not torch.equal(fresh.layer1[0].se.fc1.bias, sd["layer1.0.se.fc1.bias"])
    fresh.load_state_dict(sd)
    b = _trainer(fresh, 16, 32)
    assert torch.equal(a.prog.master, b.prog.master)
    assert torch.equal(a.evaluate_batch(img, lab), b.evaluate_batch(img, lab))


def test_drop_path_is_refused():
    with pytest.raises(ValueError, match="SE blocks"):
        _trainer(_model("seresnet18"), 16, 32, drop_path_rate=0.1)
