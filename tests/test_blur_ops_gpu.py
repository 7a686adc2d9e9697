"""The blur-pool kernels (csrc/blur_ops.hip) against fp64 torch on the same bf16 inputs: the forward oracle is
models.BlurPool2d (``F.pad(reflect)`` + ``F.conv2d(groups=C, stride=2)``) in fp64, the backward oracle its autograd
through a training-mode BN. bf16 outputs: 2^-8 of each reference element, plus 2^-20 of the tensor's largest -- the fp32
sums (at most 9 + 3 terms) err by a few 2^-24 of their largest term, which is not relative to the result where the terms
cancel. The BN moments (dgamma, dbeta through bn_bwd_coeff): 1e-4 norm-relative."""
import functools

import pytest
import torch

from dbx_distributed_pytorch_examples_amd.models import BlurPool2d
from dbx_distributed_pytorch_examples_amd.ops import kernels as K

pytestmark = pytest.mark.gpu
dev = torch.device("cuda")

# N, H, W, C: every tap reflected; odd, non-square, the last window over the border; even with two channel slabs;
# several row bands and column chunks per image (the halo between bands); the widest slab count
CASES = [(1, 2, 2, 64), (2, 7, 5, 64), (3, 8, 8, 128), (2, 57, 33, 64), (1, 4, 4, 512)]


def _blur64(x):  # NHWC fp64
    return BlurPool2d(x.shape[-1]).double()(x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)


def _bn(y, gamma, beta):
    mean, invstd = y.mean((0, 1, 2)), torch.rsqrt(y.var((0, 1, 2), unbiased=False) + 1e-5)
    return gamma * (y - mean) * invstd + beta, mean, invstd


@functools.lru_cache(maxsize=None)
def _case(N, H, W, C):
    """Inputs and the fp64 references of one shape, computed once on the CPU. y is nudged until y*scale + shift stays
    2^-6 of its terms away from 0, so the fp32 and the fp64 ReLU masks cannot disagree; about half of it is masked."""
    g = torch.Generator().manual_seed(N * 1000 + H * 100 + W * 10 + C)
    y = torch.randn(N, H, W, C, generator=g).bfloat16()
    gamma, beta = (0.5 + torch.rand(C, generator=g)).double(), (0.2 * torch.randn(C, generator=g)).double()
    for _ in range(20):
        a, mean, invstd = _bn(y.double(), gamma, beta)
        scale, shift = (gamma * invstd).float(), (beta - gamma * invstd * mean).float()
        a32 = y.double() * scale.double() + shift.double()
        margin = 2.0 ** -6 * ((y.double() * scale.double()).abs() + shift.double().abs())
        bad = a32.abs() <= 2 * margin
        if not bad.any():
            break
        y = torch.where(bad, (y.double() + torch.sign(a32 + 1e-30) * 8 * margin / scale.double()).bfloat16(), y)
    assert not bad.any() and 0.25 < (a32 > 0).double().mean() < 0.75  # the reference alone: margin and mask
    P, Q = K.blur_out_hw(H, W)
    dpool = torch.randn(N, P, Q, C, generator=g).bfloat16()
    y64, gam, bet = y.double().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    out_bn, out_plain = _blur64(torch.relu(_bn(y64, gam, bet)[0])), _blur64(y64)
    dy, dgamma, dbeta = torch.autograd.grad(out_bn, (y64, gam, bet), dpool.double())
    dx, = torch.autograd.grad(out_plain, y64, dpool.double())
    t = lambda v, dt=None: v.detach().to(dev, dt)  # noqa: E731
    return dict(y=t(y), dpool=t(dpool), scale=t(scale), shift=t(shift), gamma=t(gamma, torch.float32),
                mean=t(mean, torch.float32), invstd=t(invstd, torch.float32), out_bn=t(out_bn), out_plain=t(out_plain),
                dx=t(dx), dy=t(dy), dgamma=t(dgamma), dbeta=t(dbeta), P=P, Q=Q)


def _nan(*s, dtype=torch.bfloat16):
    return torch.full(s, float("nan"), device=dev, dtype=dtype)


def _close(out, ref, what):
    err = (out.double() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -20 * ref.abs().max()
    print(what, "worst error / bound", (err / bound).max().item())
    assert (err <= bound).all(), what


@pytest.mark.parametrize("case", CASES, ids=str)
def test_blur_fwd_and_bwd(case):
    N, H, W, C = case
    d = _case(*case)
    for kw, ref in ((dict(scale=d["scale"], shift=d["shift"]), d["out_bn"]), ({}, d["out_plain"])):
        out, again = _nan(N, d["P"], d["Q"], C), _nan(N, d["P"], d["Q"], C)
        K.blur_fwd(d["y"], out, **kw), K.blur_fwd(d["y"], again, **kw)
        _close(out, ref, f"blur_fwd {case} {sorted(kw)}")
        assert torch.equal(out, again)
    dx, again = _nan(N, H, W, C), _nan(N, H, W, C)
    K.blur_bwd(d["dpool"], dx), K.blur_bwd(d["dpool"], again)
    _close(dx, d["dx"], f"blur_bwd {case}")
    assert torch.equal(dx, again)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_blur_bn_bwd(case):
    """The reduce form's moments through bn_bwd_coeff (dgamma, dbeta), then the apply form's dy, against fp64 autograd of
    blur(relu(bn(y))) with the batch statistics inside the graph."""
    N, H, W, C = case
    d = _case(*case)
    runs = []
    for _ in range(2):
        stats = K.new_stats(C, dev, nshard=4)
        K.blur_bn_bwd_reduce(d["dpool"], d["y"], d["scale"], d["shift"], d["mean"], d["invstd"], stats)
        coeff, dgamma, dbeta = _nan(3 * C, dtype=torch.float32), _nan(C, dtype=torch.float32), _nan(C, dtype=torch.float32)
        K.bn_bwd_coeff(stats, N * H * W, d["gamma"], d["mean"], d["invstd"], coeff, dgamma, dbeta)
        dy = _nan(N, H, W, C)
        K.blur_bn_bwd_apply(d["dpool"], d["y"], d["scale"], d["shift"], coeff, dy)
        runs.append((stats, dgamma, dbeta, dy))
    (stats, dgamma, dbeta, dy), again = runs
    assert all(torch.equal(a, b) for a, b in zip(runs[0], again))
    rel = lambda a, ref: ((a.double() - ref).norm() / ref.norm()).item()  # noqa: E731
    print("moments", case, rel(dgamma, d["dgamma"]), rel(dbeta, d["dbeta"]))
    assert rel(dgamma, d["dgamma"]) < 1e-4 and rel(dbeta, d["dbeta"]) < 1e-4
    _close(dy, d["dy"], f"blur_bn_bwd_apply {case}")
