"""ResNeXt / Wide ResNet: the module trees, the reference grouped-conv ops and the program on the CPU reference ops."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig
from dbx_distributed_pytorch_examples_amd.engine.program import ResNetProgram
from dbx_distributed_pytorch_examples_amd.models import build_model
from dbx_distributed_pytorch_examples_amd.models.resnet import Bottleneck, ResNet
from dbx_distributed_pytorch_examples_amd.ops import kernels as K

CPU = torch.device("cpu")


@pytest.mark.parametrize("name,count", [("resnext50_32x4d", 25_028_904), ("resnext101_32x8d", 88_791_336),
                                        ("resnext101_64x4d", 83_455_272), ("wide_resnet50_2", 68_883_240),
                                        ("wide_resnet101_2", 126_886_696), ("resnet50", 25_557_032)])
def test_parameter_counts(name, count):
    assert sum(p.numel() for p in build_model(name).parameters()) == count


def test_state_dict_shapes():
    sd = build_model("resnext50_32x4d").state_dict()
    ref = build_model("resnet50").state_dict()
    assert list(sd) == list(ref)  # same keys, same order
    assert tuple(sd["layer1.0.conv2.weight"].shape) == (128, 4, 3, 3)
    assert tuple(sd["layer4.2.conv2.weight"].shape) == (1024, 32, 3, 3)
    assert tuple(sd["layer1.0.conv1.weight"].shape) == (128, 64, 1, 1)
    assert tuple(sd["layer1.0.conv3.weight"].shape) == (256, 128, 1, 1)
    assert tuple(ref["layer1.0.conv2.weight"].shape) == (64, 64, 3, 3)
    assert tuple(build_model("wide_resnet50_2").state_dict()["layer1.0.conv2.weight"].shape) == (128, 128, 3, 3)


@pytest.mark.parametrize("C,groups,stride", [(64, 16, 1), (64, 4, 2), (128, 2, 2)])
def test_reference_ops_match_autograd(C, groups, stride):
    torch.manual_seed(0)
    cpg = C // groups
    x = torch.randn(2, 7, 6, C).bfloat16()
    w = (torch.randn(C, 9 * cpg) / (9 * cpg) ** 0.5).bfloat16()
    xa = x.float().permute(0, 3, 1, 2).requires_grad_()
    wa = w.float().view(C, 3, 3, cpg).permute(0, 3, 1, 2).requires_grad_()
    y = F.conv2d(xa, wa, stride=stride, padding=1, groups=groups)
    dy = torch.randn_like(y).bfloat16().float()
    y.backward(dy)
    dyh = dy.permute(0, 2, 3, 1).bfloat16().contiguous()
    out, dx = torch.empty_like(dyh), torch.empty_like(x)
    stats = K.new_stats(C, CPU, nshard=2)
    K.group_conv_fwd(x, w, out, groups=groups, stride=stride, stats=stats)
    assert torch.equal(out, y.detach().permute(0, 2, 3, 1).bfloat16())
    torch.testing.assert_close(stats.view(2, 2, C).sum(0)[0], out.double().sum((0, 1, 2)))
    K.group_conv_dgrad(dyh, w, dx, groups=groups, stride=stride)
    torch.testing.assert_close(dx.float(), xa.grad.permute(0, 2, 3, 1), rtol=2 ** -7, atol=1e-3)
    dw = torch.ones(C, 9 * cpg)
    K.group_conv_wgrad(dyh, x, dw, None, groups=groups, stride=stride, scale=2.0, accumulate=True)
    torch.testing.assert_close(dw, 1 + 2 * wa.grad.permute(0, 2, 3, 1).reshape(C, -1), rtol=1e-4, atol=1e-4)


def test_program_steps_grouped_model_on_cpu():
    torch.manual_seed(0)
    model = ResNet(Bottleneck, [1, 1, 1, 1], num_classes=10, groups=32, width_per_group=4)
    tr = NativeTrainer(model, 4, (32, 32), CPU, optim=OptimConfig(lr=0.05, momentum=0.9), use_graphs=False)
    p = tr.prog
    c2 = p.blocks[0].convs[1]
    assert (c2.groups, c2.cpg, tuple(c2.grad.shape), c2.wt16) == (32, 4, (128, 36), None)
    assert dict((n, k) for n, _, k in p.param_ranges)["layer1.0.conv2.weight"] == 128 * 4 * 9
    g = torch.Generator().manual_seed(3)
    img = torch.randint(0, 256, (4, 32, 32, 3), dtype=torch.uint8, generator=g)
    lab = torch.randint(0, 10, (4,), generator=g)
    losses = []
    for _ in range(6):
        tr.step(img, lab)
        losses.append(tr.read_metrics()[0] / 4)
    assert losses[-1] < losses[0], losses
    assert model.layer1[0].conv2.weight.data_ptr() == p.master[c2.off:].data_ptr()


@pytest.mark.parametrize("conv", [nn.Conv2d(64, 64, 3, padding=2, dilation=2, bias=False),
                                  nn.Conv2d(64, 64, 1, groups=4, bias=False),
                                  nn.Conv2d(64, 64, 3, padding=1, groups=32, bias=False)],
                         ids=["dilated", "grouped_1x1", "cpg_2"])
def test_unsupported_convs_are_refused(conv):
    model = build_model("resnet50", num_classes=10)
    model.layer1[1].conv2 = conv
    with pytest.raises(TypeError):
        ResNetProgram(model, 2, (32, 32), CPU)
