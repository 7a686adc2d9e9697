"""Anti-aliased ResNets (blur_pool) through the native program on the GPU: against fp32 autograd with the damping and
the criteria of tests/test_program_gpu.py::test_program_matches_autograd (and evaluation), captured against eager,
training, and a model without the option against the same step of the same weights."""
import copy

import pytest
import torch
import torch.nn.functional as F
from test_se_program_gpu import _batch, _cos, _trainer

from dbx_distributed_pytorch_examples_amd.engine.native_trainer import OptimConfig
from dbx_distributed_pytorch_examples_amd.models import Bottleneck, ResNet, build_model

pytestmark = pytest.mark.gpu
dev = torch.device("cuda")


def _model(arch, classes=100, **kw):
    torch.manual_seed(0)
    m = (ResNet(Bottleneck, [1, 1, 1, 1], num_classes=classes, blur_pool=True, **kw) if arch == "resnetblur50"
         else build_model(arch, num_classes=classes, **kw))
    for n_, m_ in m.named_modules():  # test_program_matches_autograd's damping: last-BN gamma = 0.2
        if n_.endswith("bn3") or (n_.endswith("bn2") and "layer" in n_ and "18" in arch):
            torch.nn.init.constant_(m_.weight, 0.2)
    return m


@pytest.mark.parametrize("arch,size,kw", [("resnetblur18", 32, {}), ("resnetblur50", 64, {}),
                                           ("resnetblur50", 64, dict(groups=32, width_per_group=4, se_reduction=16))],
                         ids=["resnetblur18", "resnetblur50", "seresnextblur50"])
def test_blur_program_matches_autograd(arch, size, kw):
    model = _model(arch, **kw)
    ref = copy.deepcopy(model).to(dev).train()
    tr = _trainer(model, 8, size)
    p = tr.prog
    img, lab = _batch(8, size, p.num_classes)
    tr.step(img, lab)
    torch.cuda.synchronize()
    loss_native = p.metrics[0].item() / 8
    logits = ref(p.x4[..., :3].float().permute(0, 3, 1, 2).contiguous())
    loss = F.cross_entropy(logits, lab)
    loss.backward()
    print(arch, "loss", loss_native, loss.item(), "logits", _cos(p.logits, logits))
    assert abs(loss_native - loss.item()) / loss.item() < 3e-2 and _cos(p.logits, logits) > 0.98
    named_ref = dict(ref.named_parameters())
    for name, prm in model.named_parameters():
        off = (prm.data_ptr() - p.master.data_ptr()) // 4
        gflat = p.grad[off:off + prm.numel()]
        gn = (gflat.view(prm.shape[0], prm.shape[2], prm.shape[3], prm.shape[1]).permute(0, 3, 1, 2) if prm.dim() == 4
              else gflat.view(prm.shape))
        c = _cos(gn, named_ref[name].grad)
        assert c > (0.9 if prm.dim() > 1 else 0.75), (name, c)
    for (n1, b1), (n2, b2) in zip(model.named_buffers(), ref.named_buffers()):
        if "running_mean" in n1:
            assert _cos(b1, b2) > 0.99 or b2.abs().max() < 1e-3, n1
    # evaluation (the learning rate is 0: the same weights, and both sides' running statistics took the same step)
    out = tr.evaluate_batch(img, lab).float()
    with torch.no_grad():
        want = ref.eval()(p.x4[..., :3].float().permute(0, 3, 1, 2).contiguous())
    assert _cos(out, want) > 0.98, _cos(out, want)


@pytest.mark.parametrize("arch,size,other", [("resnetblur50", 64, dict(use_graphs=True)), ("resnet18", 32, None)],
                         ids=["captured-equals-eager", "option-off-equals-no-option"])
def test_steps_are_bit_identical(arch, size, other):
    # (option off against no option: the program tests have no launch-name hook to compare sequences with)
    opt = OptimConfig(lr=0.05, momentum=0.9, weight_decay=1e-4)
    a = _trainer(_model(arch), 8, size, optim=opt)
    b = _trainer(_model(arch, blur_pool=False), 8, size, optim=opt) if other is None else \
        _trainer(_model(arch), 8, size, optim=opt, **other)
    if other is None:
        assert b.prog.pfull is None and all(blk.blur is None for blk in b.prog.blocks)
    for i in range(3):
        img, lab = _batch(8, size, 100, seed=10 + i)
        a.step(img, lab)
        b.step(img, lab)
        torch.cuda.synchronize()
        assert torch.equal(a.prog.grad, b.prog.grad) and torch.equal(a.prog.master, b.prog.master), i


def test_sgd_learns():
    # a learnable synthetic task: the label is the brightest image quadrant
    tr = _trainer(_model("resnetblur18", classes=4), 16, 32, optim=OptimConfig(lr=0.05, momentum=0.9))
    g = torch.Generator().manual_seed(3)
    losses = []
    for _ in range(20):
        lab = torch.randint(0, 4, (16,), generator=g)
        img = torch.randint(0, 96, (16, 32, 32, 3), dtype=torch.uint8, generator=g)
        for n, q in enumerate(lab.tolist()):
            img[n, (q // 2) * 16:(q // 2) * 16 + 16, (q % 2) * 16:(q % 2) * 16 + 16] += 128
        tr.step(img.to(dev), lab.to(dev))
        losses.append(tr.read_metrics()[0] / 16)
    assert torch.isfinite(tr.prog.master).all() and sum(losses[-3:]) < 0.7 * sum(losses[:3]), losses
