"""The DropBlock kernels (csrc/dropblock_ops.hip). The mask against the numpy twin, bit for bit; the forward and the two
backward forms against fp64 torch autograd of relu(bn(y)) * keep * scale through a training-mode BN, with the bounds
of tests/test_blur_ops_gpu.py for the same arithmetic: 2^-8 of each forward element, 2^-8 of each backward element
plus 2^-20 of the tensor's largest, the BN moments (dgamma, dbeta through bn_bwd_coeff) 1e-4 norm-relative."""
import functools

import pytest
import torch
from test_blur_ops_gpu import _bn, _close, _nan

from dbx_distributed_pytorch_examples_amd.ops import kernels as K
from dbx_distributed_pytorch_examples_amd.ops import reference as R

pytestmark = pytest.mark.gpu
dev = torch.device("cuda")
SEED, OFFSET, SITE = 0x1234567887654321, 5, 3

# N, H, W, C, block size, gamma scale: one valid seed position; an odd map; layer3's setting; non-square, and there with
# the block size clipped to 6 and made odd (5); three row bands with a 3-row halo; two column chunks
SHAPES = [(1, 3, 3, 64, 3, 1.0), (3, 7, 7, 128, 3, 1.0), (3, 14, 14, 128, 5, 0.25), (1, 9, 6, 64, 5, 1.0),
          (3, 9, 6, 128, 7, 1.0), (3, 40, 7, 64, 7, 1.0), (1, 3, 40, 128, 3, 1.0)]


@functools.lru_cache(maxsize=None)
def _case(N, H, W, C, block_size, gamma_scale, p):
    """Inputs, the twin's mask and the fp64 references of one case, computed once on the CPU. y is nudged as in
    test_blur_ops_gpu until y*scale + shift stays 2^-6 of its terms away from 0 (the ReLU masks cannot disagree)."""
    bs, gamma = R.dropblock_geometry(H, W, block_size, p, gamma_scale)
    thr = R.dropblock_threshold(gamma)
    bits, kept = R.dropblock_mask(N, H, W, C, thr, block_size, SEED, OFFSET, SITE)
    assert 0 < kept < N * H * W * C  # (the seeds above keep something and drop something in every case)
    g = torch.Generator().manual_seed(N * 1000 + H * 100 + W * 10 + C)
    y = torch.randn(N, H, W, C, generator=g).bfloat16()
    gamma_, beta = (0.5 + torch.rand(C, generator=g)).double(), (0.2 * torch.randn(C, generator=g)).double()
    for _ in range(20):
        a, mean, invstd = _bn(y.double(), gamma_, beta)
        scale, shift = (gamma_ * invstd).float(), (beta - gamma_ * invstd * mean).float()
        a32 = y.double() * scale.double() + shift.double()
        margin = 2.0 ** -6 * ((y.double() * scale.double()).abs() + shift.double().abs())
        bad = a32.abs() <= 2 * margin
        if not bad.any():
            break
        y = torch.where(bad, (y.double() + torch.sign(a32 + 1e-30) * 8 * margin / scale.double()).bfloat16(), y)
    assert not bad.any()
    das = torch.randn(N, H, W, C, generator=g).bfloat16()
    m = R.dropblock_unpack(bits, C).double() * R.dropblock_scale(N * H * W * C, kept)
    y64, gam, bet = y.double().requires_grad_(), gamma_.clone().requires_grad_(), beta.clone().requires_grad_()
    out = torch.relu(_bn(y64, gam, bet)[0]) * m
    dy, dgamma, dbeta = torch.autograd.grad(out, (y64, gam, bet), das.double())
    t = lambda v, dt=None: v.detach().to(dev, dt)  # noqa: E731
    return dict(y=t(y), das=t(das), scale=t(scale), shift=t(shift), gamma=t(gamma_, torch.float32),
                mean=t(mean, torch.float32), invstd=t(invstd, torch.float32), out=t(out), dy=t(dy), dgamma=t(dgamma),
                dbeta=t(dbeta), bits=t(bits), kept=kept,
                thr=torch.tensor([thr - (1 << 32) if thr >= 1 << 31 else thr], dtype=torch.int32, device=dev),
                off=torch.tensor([OFFSET], dtype=torch.int32, device=dev))


@pytest.mark.parametrize("p", [0.1, 0.9])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_dropblock_kernels(shape, p):
    N, H, W, C, block_size, _ = shape
    d = _case(*shape, p)
    runs = []
    for _ in range(2):
        bits = torch.full((N, H, W, C // 32), 0x55555555, device=dev, dtype=torch.int32)
        kept = torch.zeros(1, device=dev, dtype=torch.int64)
        K.dropblock_mask(bits, kept, d["thr"], d["off"], block_size=block_size, seed=SEED, site=SITE)
        out = K.dropblock_fwd(d["y"], d["scale"], d["shift"], bits, kept, _nan(N, H, W, C))
        stats = K.new_stats(C, dev, nshard=4)
        K.dropblock_bn_bwd_reduce(d["das"], d["y"], d["scale"], d["shift"], bits, kept, d["mean"], d["invstd"], stats)
        coeff, dgamma, dbeta = _nan(3 * C, dtype=torch.float32), _nan(C, dtype=torch.float32), _nan(C, dtype=torch.float32)
        K.bn_bwd_coeff(stats, N * H * W, d["gamma"], d["mean"], d["invstd"], coeff, dgamma, dbeta)
        dy = _nan(N, H, W, C)
        K.dropblock_bn_bwd_apply(d["das"], d["y"], d["scale"], d["shift"], bits, kept, coeff, dy)
        runs.append((bits, kept, out, stats, dgamma, dbeta, dy))
    (bits, kept, out, stats, dgamma, dbeta, dy), again = runs
    assert all(torch.equal(a, b) for a, b in zip(runs[0], again))
    assert kept.item() == d["kept"] and torch.equal(bits, d["bits"])
    err = (out.double() - d["out"]).abs()
    print("fwd", shape, p, "kept", d["kept"], "worst error / bound", (err / (2.0 ** -8 * d["out"].abs() + 1e-300)).max().item())
    assert (err <= 2.0 ** -8 * d["out"].abs()).all()
    rel = lambda a, ref: ((a.double() - ref).norm() / ref.norm()).item()  # noqa: E731
    print("moments", rel(dgamma, d["dgamma"]), rel(dbeta, d["dbeta"]))
    assert rel(dgamma, d["dgamma"]) < 1e-4 and rel(dbeta, d["dbeta"]) < 1e-4
    _close(dy, d["dy"], f"dropblock_bn_bwd_apply {shape} {p}")
