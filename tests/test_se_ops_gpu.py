"""The squeeze-and-excitation kernels (csrc/se_ops.hip) against fp64 torch on the same bf16 inputs. bf16 outputs within
2^-8 norm-relative, fp32 outputs within 1e-4; gate / dpre2 / dpre1 / dz sit behind the bf16-stored zq / h and get 2^-8
(the reference rounds z and h where the kernel does)."""
import pytest
import torch

from dbx_distributed_pytorch_examples_amd.ops import kernels as K

pytestmark = pytest.mark.gpu
dev = torch.device("cuda")

# N, H, W, C, rd: one pixel and N < the 16-sample tile; an odd map with rd below the MFMA tile; the row-split
# reductions (more than 256 pixels); the widest C, the largest rd of the named models and a ragged second sample tile
CASES = [(3, 1, 1, 64, 8), (5, 7, 7, 128, 8), (2, 56, 56, 64, 8), (17, 4, 4, 2048, 128)]
BF, F32 = 2 ** -8, 1e-4


def _rel(a, ref):
    return ((a.double() - ref).norm() / ref.norm().clamp_min(1e-30)).item()


def _inputs(N, H, W, C, rd):
    g = torch.Generator().manual_seed(N * 1000 + H * 100 + C + rd)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    d = dict(y=r(N, H, W, C).bfloat16(), g=r(N, H, W, C).bfloat16(), res=r(N, H, W, C).bfloat16(),
             scale=0.5 + torch.rand(C, generator=g), shift=0.3 * r(C), mean=0.2 * r(C), invstd=0.5 + torch.rand(C, generator=g),
             gamma=0.5 + torch.rand(C, generator=g), beta=0.3 * r(C), rsc=0.5 + torch.rand(C, generator=g), rsh=0.3 * r(C),
             w1=(r(rd, C) / C ** 0.5).bfloat16(), b1=0.1 * r(rd), w2=(r(C, rd) / rd ** 0.5).bfloat16(), b2=0.1 * r(C))
    return {k: v.to(dev) for k, v in d.items()}


def _z(*s, dtype=torch.float32):
    return torch.full(s, float("nan"), device=dev, dtype=dtype)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_forward(case):
    N, H, W, C, rd = case
    d, HW = _inputs(*case), H * W
    zsum, zq, h, gate = _z(N, C), _z(N, C, dtype=torch.bfloat16), _z(N, rd, dtype=torch.bfloat16), _z(N, C)
    K.se_squeeze(d["y"], zsum)
    again = K.se_squeeze(d["y"], torch.zeros_like(zsum))
    assert torch.equal(zsum, again)
    y64 = d["y"].double()
    assert _rel(zsum, y64.reshape(N, HW, C).sum(1)) < F32
    K.se_excite(zsum, d["scale"], d["shift"], HW, d["w1"], d["b1"], d["w2"], d["b2"], zq, h, gate)
    zq_ref = d["scale"].double() * zsum.double() / HW + d["shift"].double()
    assert _rel(zq, zq_ref) < BF
    h_ref = torch.relu(zq.double() @ d["w1"].double().t() + d["b1"].double())
    assert _rel(h, h_ref) < BF
    gate_ref = torch.sigmoid(h.double() @ d["w2"].double().t() + d["b2"].double())
    assert _rel(gate, gate_ref) < BF
    u = gate.double().view(N, 1, 1, C) * (d["scale"].double() * y64 + d["shift"].double())
    for res, rsc, rsh in ((None, None, None), (d["res"], None, None), (d["res"], d["rsc"], d["rsh"])):
        out, bits = _z(N, H, W, C, dtype=torch.bfloat16), torch.zeros(N * HW * C // 8, device=dev, dtype=torch.uint8)
        K.se_tail(d["y"], d["scale"], d["shift"], gate, out, res=res, res_scale=rsc, res_shift=rsh, mbits=bits)
        r = 0 if res is None else res.double() if rsc is None else res.double() * rsc.double() + rsh.double()
        assert _rel(out, torch.relu(u + r)) < BF
        assert torch.equal(K.unpack_mask_bits(bits, out.shape), out > 0)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_backward(case):
    """Every backward kernel, and the BN moments through bn_bwd_coeff against fp64 autograd of the whole SE tail
    out = relu(res + gate * (gamma * xhat + beta)) with respect to gamma / beta. The graph rounds z and h to bf16 where
    the kernel stores them (straight through); 2^-8, since the moments contain dz, which sits behind the bf16-stored
    dpre2 / dpre1 that the graph does not round."""
    N, H, W, C, rd = case
    d, HW = _inputs(*case), H * W
    sc, sh = d["gamma"] * d["invstd"], d["beta"] - d["gamma"] * d["invstd"] * d["mean"]  # the BN's forward coefficients
    zsum, zq, h, gate = _z(N, C), _z(N, C, dtype=torch.bfloat16), _z(N, rd, dtype=torch.bfloat16), _z(N, C)
    out, bits = _z(N, H, W, C, dtype=torch.bfloat16), torch.zeros(N * HW * C // 8, device=dev, dtype=torch.uint8)
    K.se_squeeze(d["y"], zsum)
    K.se_excite(zsum, sc, sh, HW, d["w1"], d["b1"], d["w2"], d["b2"], zq, h, gate)
    K.se_tail(d["y"], sc, sh, gate, out, res=d["res"], mbits=bits)
    A, B = _z(N, C), _z(N, C)
    K.se_bwd_reduce(d["g"], bits, d["y"], d["mean"], d["invstd"], A, B)
    A2, B2 = torch.zeros_like(A), torch.zeros_like(B)
    K.se_bwd_reduce(d["g"], bits, d["y"], d["mean"], d["invstd"], A2, B2)
    assert torch.equal(A, A2) and torch.equal(B, B2)
    gm = d["g"].double() * (out > 0)
    xhat = (d["y"].double() - d["mean"].double()) * d["invstd"].double()
    assert _rel(A, gm.reshape(N, HW, C).sum(1)) < F32
    assert _rel(B, (gm * xhat).reshape(N, HW, C).sum(1)) < F32
    dpre2, dpre1, dz = _z(N, C, dtype=torch.bfloat16), _z(N, rd, dtype=torch.bfloat16), _z(N, C)
    bst = torch.full((4 * 2 * C,), 7.0, device=dev, dtype=torch.float64)
    K.se_excite_bwd(A, B, gate, h, zsum, HW, d["gamma"], d["beta"], d["mean"], d["invstd"], d["w2"], d["w1"], dpre2,
                    dpre1, dz, bst)
    bst2 = torch.zeros_like(bst)
    K.se_excite_bwd(A, B, gate, h, zsum, HW, d["gamma"], d["beta"], d["mean"], d["invstd"], d["w2"], d["w1"], dpre2,
                    dpre1, dz, bst2)
    assert torch.equal(bst, bst2) and not bst.view(4, 2, C)[1:].any()
    g64 = gate.double()
    dp2 = (d["gamma"].double() * B.double() + d["beta"].double() * A.double()) * g64 * (1 - g64)
    assert _rel(dpre2, dp2) < BF
    dp1 = (dpre2.double() @ d["w2"].double()) * (h > 0)
    assert _rel(dpre1, dp1) < BF
    assert _rel(dz, dpre1.double() @ d["w1"].double()) < BF
    coeff, dgam, dbet = _z(3 * C), _z(C), _z(C)
    K.bn_bwd_coeff(bst, N * HW, d["gamma"], d["mean"], d["invstd"], coeff, dgam, dbet)
    dy, gout = _z(N, H, W, C, dtype=torch.bfloat16), _z(N, H, W, C, dtype=torch.bfloat16)
    K.se_bwd_apply(d["g"], bits, d["y"], gate, dz, coeff, dy, gout)
    assert torch.equal(gout, (d["g"].float() * (out > 0)).bfloat16())
    k = coeff.double().view(3, C)
    du = gm * g64.view(N, 1, 1, C) + dz.double().view(N, 1, 1, C) / HW
    assert _rel(dy, k[0] * du + k[1] * d["y"].double() + k[2]) < BF
    # fp64 autograd of the tail (the gate as a function of the BN output; the mask taken from the kernel's output)
    rq = lambda t: t + (t.float().bfloat16().double() - t).detach()  # noqa: E731
    gam, bet = d["gamma"].double().requires_grad_(), d["beta"].double().requires_grad_()
    u = gam * xhat + bet
    hh = rq(torch.relu(rq(u.reshape(N, HW, C).mean(1)) @ d["w1"].double().t() + d["b1"].double()))
    s = torch.sigmoid(hh @ d["w2"].double().t() + d["b2"].double())
    ((s.view(N, 1, 1, C) * u) * gm).sum().backward()
    print("moments", case, _rel(dgam, gam.grad), _rel(dbet, bet.grad))
    assert _rel(dgam, gam.grad) < BF and _rel(dbet, bet.grad) < BF


def test_bad_arguments_raise_before_a_launch():
    y = torch.zeros(2, 4, 4, 96, device=dev, dtype=torch.bfloat16)  # C % 64 != 0
    with pytest.raises(ValueError):
        K.se_squeeze(y, torch.zeros(2, 96, device=dev))
    y = torch.zeros(2, 4, 4, 64, device=dev, dtype=torch.bfloat16)
    f = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    with pytest.raises(ValueError):  # rd = 4
        K.se_excite(f(2, 64), f(64), f(64), 16, y.new_zeros(4, 64), f(4), y.new_zeros(64, 4), f(64), y.new_zeros(2, 64),
                    y.new_zeros(2, 4), f(2, 64))
    with pytest.raises(ValueError):  # a mask of the wrong length
        K.se_tail(y, f(64), f(64), f(2, 64), torch.empty_like(y), mbits=torch.zeros(7, device=dev, dtype=torch.uint8))
