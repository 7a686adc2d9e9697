"""SE-ResNet on the CPU: the module trees, the reference twins of the SE kernels, the program's parameter layout."""
import pytest
import torch

from dbx_distributed_pytorch_examples_amd.models import Bottleneck, ResNet, build_model
from dbx_distributed_pytorch_examples_amd.ops import reference as R


@pytest.mark.parametrize("name,count", [("seresnet50", 28_088_024), ("seresnext50_32x4d", 27_559_896)])
def test_parameter_counts_and_keys(name, count):
    m = build_model(name)
    assert sum(p.numel() for p in m.parameters()) == count
    keys = set(m.state_dict())
    assert {"layer1.0.se.fc1.weight", "layer1.0.se.fc1.bias", "layer4.2.se.fc2.weight", "layer4.2.se.fc2.bias"} <= keys
    assert m.layer1[0].se.fc1.weight.shape == (16, 256, 1, 1) and m.layer4[2].se.fc2.weight.shape == (2048, 128, 1, 1)


def test_no_reduction_is_the_plain_model():
    torch.manual_seed(5)
    a = build_model("resnet50", num_classes=10)
    torch.manual_seed(5)
    b = ResNet(Bottleneck, [3, 4, 6, 3], num_classes=10, se_reduction=0)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and not any(".se." in k for k in sb) and not hasattr(b.layer1[0], "se")
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert torch.equal(torch.rand(3), (torch.manual_seed(5), build_model("resnet50", num_classes=10), torch.rand(3))[2])


def test_reference_twins_match_a_direct_formulation():
    torch.manual_seed(0)
    N, H, W, C, rd = 3, 5, 5, 64, 8
    y = torch.randn(N, H, W, C).bfloat16()
    scale, shift = torch.rand(C) + 0.5, torch.randn(C) * 0.2
    w1, b1, w2, b2 = (torch.randn(rd, C) / 8).bfloat16(), torch.randn(rd) * 0.1, (torch.randn(C, rd) / 3).bfloat16(), torch.randn(C) * 0.1
    zsum, zq, h, gate = torch.zeros(N, C), torch.zeros(N, C).bfloat16(), torch.zeros(N, rd).bfloat16(), torch.zeros(N, C)
    out, bits = torch.zeros_like(y), torch.zeros(y.numel() // 8, dtype=torch.uint8)
    R.se_squeeze(y, zsum)
    R.se_excite(zsum, scale, shift, H * W, w1, b1, w2, b2, zq, h, gate)
    R.se_tail(y, scale, shift, gate, out, res=y, mbits=bits)
    u = (y.float() * scale + shift).permute(0, 3, 1, 2)
    z = u.mean((2, 3), keepdim=True)
    s = torch.sigmoid(torch.nn.functional.conv2d(torch.relu(torch.nn.functional.conv2d(z, w1.float().view(rd, C, 1, 1), b1)),
                                                 w2.float().view(C, rd, 1, 1), b2))
    want = torch.relu(u * s + y.float().permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    torch.testing.assert_close(out.float(), want, rtol=2e-2, atol=2e-2)
    # backward twins against autograd of the same tail in terms of the gate's pre-activations and y
    g = torch.randn(N, H, W, C).bfloat16()
    mean, invstd, gamma = torch.randn(C) * 0.1, torch.rand(C) + 0.5, torch.rand(C) + 0.5
    beta = shift + gamma * invstd * mean  # so that scale = gamma * invstd reproduces shift
    scale = gamma * invstd
    R.se_squeeze(y, zsum)
    R.se_excite(zsum, scale, shift, H * W, w1, b1, w2, b2, zq, h, gate)
    R.se_tail(y, scale, shift, gate, out, res=y, mbits=bits)
    A, B, dz = torch.zeros(N, C), torch.zeros(N, C), torch.zeros(N, C)
    dpre2, dpre1, bst = torch.zeros(N, C).bfloat16(), torch.zeros(N, rd).bfloat16(), torch.zeros(2 * 2 * C, dtype=torch.float64)
    R.se_bwd_reduce(g, bits, y, mean, invstd, A, B)
    R.se_excite_bwd(A, B, gate, h, zsum, H * W, gamma, beta, mean, invstd, w2, w1, dpre2, dpre1, dz, bst)
    gam = gamma.double().requires_grad_()
    xhat = (y.double() - mean.double()) * invstd.double()
    u = gam * xhat + beta.double()
    hh = torch.relu(u.reshape(N, -1, C).mean(1) @ w1.double().t() + b1.double())
    sg = torch.sigmoid(hh @ w2.double().t() + b2.double())
    ((sg.view(N, 1, 1, C) * u) * (g.double() * (out > 0))).sum().backward()
    torch.testing.assert_close(bst.view(2, 2, C)[0, 1], gam.grad, rtol=2e-2, atol=2e-2)


def test_program_compiles_an_se_model_on_the_cpu():
    from dbx_distributed_pytorch_examples_amd.engine.program import ResNetProgram
    m = ResNet(Bottleneck, [1, 1, 1, 1], num_classes=10, se_reduction=16)
    p = ResNetProgram(m, 2, (32, 32), torch.device("cpu"))
    names = [r[0] for r in p.param_ranges]
    for li in range(1, 5):
        seg = [n for n in names if n.startswith(f"layer{li}.")]
        lo, hi = names.index(seg[0]), names.index(seg[-1])
        assert hi - lo + 1 == len(seg)  # one contiguous run of the flat buffer
        assert {f"layer{li}.0.se.fc1.weight", f"layer{li}.0.se.fc1.bias", f"layer{li}.0.se.fc2.weight",
                f"layer{li}.0.se.fc2.bias"} <= set(seg)
    assert m.layer1[0].se.fc1.weight.data_ptr() == p.master[p.blocks[0].se.off["fc1.weight"]:].data_ptr()
    p.enable_drop_path([0.0] * 4)
    with pytest.raises(ValueError, match="SE blocks"):
        p.enable_drop_path([0.0, 0.1, 0.0, 0.0])
    m.layer1[0].se.fc1 = torch.nn.Conv2d(256, 12, 1)  # rd = 12: not a multiple of 8
    m.layer1[0].se.fc2 = torch.nn.Conv2d(12, 256, 1)
    with pytest.raises(TypeError, match="squeezed width"):
        ResNetProgram(m, 2, (32, 32), torch.device("cpu"))
