"""Per-element checks of the memory-bound kernels (csrc/nn_ops.hip, csrc/input_ops.hip) at every width and option.

Every test runs on the CPU (``ops.kernels`` dispatches CPU tensors to ``ops/reference.py``, so the
test's own logic and bounds are checked without a GPU, and the reference path is pinned) and on the
GPU (the HIP kernel). The oracle is always plain float64 torch of the textbook formula, written
here; it is never ``reference.py`` and never another kernel.

Bounds (derived, per element; no norm ratios):

* bf16 output of an fp32 elementwise chain: ``|got - ref| <= 2^-8 |ref| + 2^-20 mag`` with ``mag`` the
  sum of the absolute values of the chain's terms (2^-8: bf16's unit roundoff; 2^-20: 16 fp32
  roundings, which covers any FMA contraction and operation order);
* fp32 output of an elementwise chain: ``|got - ref| <= 2^-20 mag``;
* a sum of n fp32 terms: ``|got - ref| <= (n 2^-24 + 2^-21) sum|term|`` (any summation order);
* pure moves and casts: bit-exact.

Widened for a documented intrinsic error (nothing else is):

* ``softmax_ce``: ``__expf(x)`` evaluates ``exp2(x * log2(e))``; the fp32 rounding of the product is an
  absolute error of ``|x| 2^-24 log2(e)`` in the exponent, i.e. a relative error of ``|x| 2^-24`` of the
  result, plus 2 ulp of the hardware exp2 (the usual ``2 + floor(1.16 |x|)`` ulp figure of the fast
  exponential). The probability term of dlogits gets ``(2 + 1.16 |x - lse|) 2^-23 p`` on top, plus the
  log-sum-exp's own error relative to p: ``(C 2^-24 + 2^-20) + (2 + 1.16 max|x - max|) 2^-23`` (a sum
  of C such exponentials; d lse = d se / se). Without it the MI355X reaches 1.72 of the plain bound.
  The loss keeps the plain fp32 bound (``__logf`` stays inside it).

Every output buffer starts filled with NaN, inside guard elements holding a sentinel bit pattern
that must be unchanged afterwards. The largest ``err / bound`` of each test is collected in
``RATIOS`` (printed at the end of the module; written as JSON to ``$DBX_NN_OPS_RATIOS`` when set).
"""
import itertools
import json
import math
import os
from types import SimpleNamespace

import pytest
import torch

from dbx_distributed_pytorch_examples_amd.ops import kernels as K

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
devices = pytest.mark.parametrize("dev", DEVICES)  # on every test
GPU_ONLY = [pytest.param("cuda", marks=pytest.mark.gpu)]  # (the grid-stride cases: the CPU path has no grid)

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U_BF16 = 2.0 ** -8     # bf16 unit roundoff
U_CHAIN = 2.0 ** -20   # 16 fp32 roundings
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    if not RATIOS:
        return
    print("\n[test_nn_ops] largest err / bound per test and device:")
    for k in sorted(RATIOS):
        print(f"  {k}: {RATIOS[k]:.4f}")
    path = os.environ.get("DBX_NN_OPS_RATIOS")
    if path:
        with open(path, "w") as f:
            json.dump(RATIOS, f, indent=1, sort_keys=True)


# ---------------------------------------------------------------------------------------------
# helpers: bounds, guarded buffers, data
# ---------------------------------------------------------------------------------------------
def bf16_bound(ref, mag):
    return U_BF16 * ref.abs() + U_CHAIN * mag


def f32_bound(mag):
    return U_CHAIN * mag


def sum_bound(n, sum_abs):
    return (n * 2.0 ** -24 + 2.0 ** -21) * sum_abs


def check(key, dev, got, ref, bound, what="", plain=None):
    """Every element of ``got`` is finite and within ``bound`` of the float64 ``ref``; records the
    largest err / bound under ``key``. ``plain``: the bound before it was widened for an intrinsic's
    documented error -- its ratio is recorded too (not asserted), to show what the widening is for."""
    got = got.detach().double().reshape(ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite (unwritten?) output elements"
    err = (got - ref).abs()
    if plain is not None:
        r = float(torch.where(err == 0, torch.zeros_like(err), err / plain).max())
        k = f"{key}[{dev}] {what.split()[-1]}, bound not widened"
        RATIOS[k] = max(RATIOS.get(k, 0.0), r)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"{key}[{dev}] {what}: max err/bound = {worst:.4f}")
    k = f"{key}[{dev}]"
    RATIOS[k] = max(RATIOS.get(k, 0.0), worst)
    if not worst <= 1.0:
        i = int(ratio.flatten().argmax())
        raise AssertionError(f"{what}: element {i}: got {got.flatten()[i].item()!r}, want {ref.flatten()[i].item()!r}, "
                             f"err {err.flatten()[i].item():.3e} > bound {bound.flatten()[i].item():.3e} "
                             f"(ratio {worst:.3f}; {int((ratio > 1).sum())} of {ratio.numel()} elements out)")


_INT = {BF: torch.int16, F32: torch.int32, F64: torch.int64, torch.uint8: torch.uint8, torch.int64: torch.int64}
_SENTINEL = {BF: 0x7FA5, F32: 0x7FC0A5A5, F64: 0x7FF8A5A5A5A5A5A5, torch.uint8: 0xA5, torch.int64: 0x5A5A5A5A5A5A5A5A}
GUARD = 64  # elements on each side (a multiple of 16 bytes for every dtype: the body keeps its alignment)


class Guarded:
    """A tensor ``t`` of ``shape`` in the middle of a larger allocation whose guard elements hold a
    sentinel bit pattern. ``t`` starts as NaN (floats) / 0xFF (bytes), or as a copy of ``init``."""

    def __init__(self, shape, dtype, dev, init=None):
        shape = tuple(shape) if not isinstance(shape, int) else (shape,)
        n = math.prod(shape)
        self.n, self.dtype = n, dtype
        self.buf = torch.empty(n + 2 * GUARD, dtype=dtype, device=dev)
        self.bits = self.buf.view(_INT[dtype])
        self.bits.fill_(_SENTINEL[dtype])
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        if init is not None:
            self.t.copy_(init.reshape(shape))
        elif dtype == torch.uint8:
            self.t.fill_(0xFF)
        elif dtype == torch.int64:
            self.t.zero_()
        else:
            self.t.fill_(float("nan"))

    def check(self, what=""):
        g = torch.cat([self.bits[:GUARD], self.bits[GUARD + self.n:]])
        assert bool((g == _SENTINEL[self.dtype]).all()), f"{what}: wrote outside the output region"


def G(shape, dtype, dev, init=None):
    return Guarded(shape, dtype, dev, init)


def gen(dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return g


def randn(g, *shape, dtype=F32, scale=1.0):
    return (torch.randn(*shape, generator=g, device=g.device, dtype=F32) * scale).to(dtype)


def rand(g, *shape, lo=0.0, hi=1.0):
    return torch.rand(*shape, generator=g, device=g.device, dtype=F32) * (hi - lo) + lo


def f32(x):
    """The float32 value a Python float becomes when passed to a kernel, as a Python float."""
    return float(torch.tensor(x, dtype=F32).double())


def pack_bits(mask):
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.int32, device=mask.device)
    return (mask.reshape(-1, 8).to(torch.int32) * w).sum(1).to(torch.uint8)


def rpb_of(C):
    return 256 // (C // 8)


CHANNELS = [8, 64, 192, 512, 2048]


def row_cases():
    """(C, M): M in {1, rpb-1, rpb+1, 37} for every C."""
    return [pytest.param(C, M, id=f"C{C}-M{M}") for C in CHANNELS
            for M in sorted({1, rpb_of(C) - 1, rpb_of(C) + 1, 37} - {0})]


def grid_stride(test, cap):
    """The GPU-only cases of a row-mapped test: cap * rpb + 3 rows at C in {8, 2048}, which takes the
    grid-stride loop of a grid capped at ``cap`` blocks round a second time."""
    @pytest.mark.parametrize("dev", GPU_ONLY)
    @pytest.mark.parametrize("C", [8, 2048])
    def run(dev, C):
        test(dev, C, cap * rpb_of(C) + 3)
    run.__name__ = run.__qualname__ = test.__name__ + "_grid_stride"
    return run


# ---------------------------------------------------------------------------------------------
# bn_apply
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,M", row_cases())
@devices
def test_bn_apply(dev, C, M):
    g = gen(dev, 1)
    y, r = randn(g, M, C, dtype=BF), randn(g, M, C, dtype=BF)
    s, h, a, b = randn(g, C), randn(g, C), randn(g, C), randn(g, C)
    y64, r64 = y.double(), r.double()
    base, bmag = y64 * s.double() + h.double(), (y64 * s.double()).abs() + h.double().abs()
    for res_mode, relu, mb in itertools.product((0, 1, 2), (False, True), (False, True)):
        if mb and not relu:
            continue
        ref, mag = base, bmag
        kw = {}
        if res_mode == 1:
            ref, mag, kw = base + r64, bmag + r64.abs(), dict(res=r)
        elif res_mode == 2:
            ref = base + r64 * a.double() + b.double()
            mag = bmag + (r64 * a.double()).abs() + b.double().abs()
            kw = dict(res=r, res_scale=a, res_shift=b)
        if relu:
            ref = ref.clamp_min(0)
        out = G((M, C), BF, dev)
        bits = G(M * C // 8, torch.uint8, dev) if mb else None
        K.bn_apply(y, s, h, out.t, relu=relu, mbits=bits.t if mb else None, **kw)
        what = f"res{res_mode} relu{int(relu)} mbits{int(mb)}"
        check("bn_apply", dev, out.t, ref, bf16_bound(ref, mag), what)
        out.check(what)
        if mb:  # the mask of the stored values, bit j of byte i = element 8i + j
            assert torch.equal(bits.t, pack_bits(out.t.float() > 0)), what
            bits.check(what)


test_bn_apply_grid_stride = grid_stride(test_bn_apply, 4096)


@pytest.mark.parametrize("C", [12, 2056])
@devices
def test_per_channel_bad_width_raises(dev, C):
    M = 4
    z = lambda dt=BF: torch.zeros(M, C, dtype=dt, device=dev)  # noqa: E731
    v = torch.ones(C, device=dev)
    st = torch.zeros(4 * 2 * C, dtype=F64, device=dev)
    co = torch.zeros(3 * C, device=dev)
    E = (ValueError, RuntimeError)
    with pytest.raises(E):
        K.bn_apply(z(), v, v, z(), relu=True)
    with pytest.raises(E):
        K.channel_stats(z(), st)
    with pytest.raises(E):
        K.bn_bwd_reduce(z(), z(), v, v, st, mask_mode=0)
    with pytest.raises(E):
        K.bn_bwd_apply(z(), z(), co, z(), mask_mode=0)
    with pytest.raises(E):
        K.bn_bwd_apply2(z(), z(), co, z(), z(), co, z())
    with pytest.raises(E):
        K.maxpool_fwd(torch.zeros(1, 2, 2, C, dtype=BF, device=dev), torch.zeros(1, 1, 1, C, dtype=BF, device=dev),
                      torch.zeros(1, 1, 1, C, dtype=torch.uint8, device=dev), K=3, stride=2, pad=1)


# ---------------------------------------------------------------------------------------------
# channel_stats, bn_bwd_reduce
# ---------------------------------------------------------------------------------------------
NSH = 4


def _slab(C, dev, nshard=NSH):
    return G(nshard * 2 * C, F64, dev, init=torch.zeros(nshard * 2 * C, dtype=F64, device=dev))


@pytest.mark.parametrize("C,M", row_cases())
@devices
def test_channel_stats(dev, C, M):
    y = randn(gen(dev, 2), M, C, dtype=BF)
    st = _slab(C, dev)
    K.channel_stats(y, st.t)
    got = st.t.view(NSH, 2, C).sum(0)
    y64 = y.double()
    check("channel_stats", dev, got[0], y64.sum(0), sum_bound(M, y64.abs().sum(0)), "sum")
    check("channel_stats", dev, got[1], (y64 * y64).sum(0), sum_bound(M, (y64 * y64).sum(0)), "sumsq")
    st.check()


test_channel_stats_grid_stride = grid_stride(test_channel_stats, 2048)


def _masked(dout, y, mref, s, h, mask_mode):
    """float64 g = dout * mask and the elements whose MASK_Y decision is within fp32 rounding of the
    threshold (there either value of the mask is right)."""
    g = dout.double()
    amb = torch.zeros_like(g, dtype=torch.bool)
    if mask_mode == 1:
        g = g * (mref.double() > 0)
    elif mask_mode == 2:
        t = y.double() * s.double() + h.double()
        amb = t.abs() <= U_CHAIN * ((y.double() * s.double()).abs() + h.double().abs())
        g = g * (t > 0)
    return g, amb


@pytest.mark.parametrize("C,M", row_cases())
@devices
def test_bn_bwd_reduce(dev, C, M):
    g = gen(dev, 3)
    dout, y, mref = randn(g, M, C, dtype=BF), randn(g, M, C, dtype=BF), randn(g, M, C, dtype=BF)
    s, h, mu, inv = randn(g, C), randn(g, C), randn(g, C), rand(g, C, lo=0.5, hi=2.0)
    for mask_mode in (0, 1, 2):
        gm, amb = _masked(dout, y, mref, s, h, mask_mode)
        term = gm * (y.double() - mu.double()) * inv.double()
        # (an element with an ambiguous mask may be in or out of the sum)
        slack_s = (dout.double().abs() * amb).sum(0)
        slack_q = ((dout.double() * (y.double() - mu.double()) * inv.double()).abs() * amb).sum(0)
        st = _slab(C, dev)
        kw = dict(mref=mref) if mask_mode == 1 else dict(scale=s, shift=h) if mask_mode == 2 else {}
        K.bn_bwd_reduce(dout, y, mu, inv, st.t, mask_mode=mask_mode, **kw)
        got = st.t.view(NSH, 2, C).sum(0)
        check("bn_bwd_reduce", dev, got[0], gm.sum(0), sum_bound(M, gm.abs().sum(0)) + slack_s, f"mask{mask_mode} sum g")
        check("bn_bwd_reduce", dev, got[1], term.sum(0), sum_bound(M, term.abs().sum(0)) + slack_q,
              f"mask{mask_mode} sum g*xhat")
        st.check()


test_bn_bwd_reduce_grid_stride = grid_stride(test_bn_bwd_reduce, 2048)


# ---------------------------------------------------------------------------------------------
# bn_bwd_apply, bn_bwd_apply2
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,M", row_cases())
@devices
def test_bn_bwd_apply(dev, C, M):
    g = gen(dev, 4)
    dout, y, mref = randn(g, M, C, dtype=BF), randn(g, M, C, dtype=BF), randn(g, M, C, dtype=BF)
    s, h, co = randn(g, C), randn(g, C), randn(g, 3 * C)
    k1, k2, k3 = co.double().view(3, C)
    for mask_mode, wg in itertools.product((0, 1, 2), (False, True)):
        gm, amb = _masked(dout, y, mref, s, h, mask_mode)
        dy, gout = G((M, C), BF, dev), (G((M, C), BF, dev) if wg else None)
        kw = dict(mref=mref) if mask_mode == 1 else dict(scale=s, shift=h) if mask_mode == 2 else {}
        K.bn_bwd_apply(dout, y, co, dy.t, mask_mode=mask_mode, gout=gout.t if wg else None, **kw)
        what = f"mask{mask_mode} gout{int(wg)}"
        if amb.any():  # take the kernel's decision where fp32 rounding decides the mask
            alt = dout.double() - gm  # the other mask value's g
            ref_a, ref_b = k1 * gm + k2 * y.double() + k3, k1 * alt + k2 * y.double() + k3
            pick = amb & ((dy.t.double() - ref_b).abs() < (dy.t.double() - ref_a).abs())
            gm = torch.where(pick, alt, gm)
        ref = k1 * gm + k2 * y.double() + k3
        mag = (k1 * gm).abs() + (k2 * y.double()).abs() + k3.abs()
        check("bn_bwd_apply", dev, dy.t, ref, bf16_bound(ref, mag), what)
        dy.check(what)
        if wg:  # a pure move: dout or zero
            ok = gout.t.double() == gm
            ok |= amb & ((gout.t.double() == 0) | (gout.t.double() == dout.double()))
            assert bool(ok.all()), f"{what}: gout differs at {int((~ok).sum())} elements"
            gout.check(what)


test_bn_bwd_apply_grid_stride = grid_stride(test_bn_bwd_apply, 4096)


@pytest.mark.parametrize("C,M", row_cases())
@devices
def test_bn_bwd_apply2(dev, C, M):
    g = gen(dev, 5)
    gi, y1, y2 = randn(g, M, C, dtype=BF), randn(g, M, C, dtype=BF), randn(g, M, C, dtype=BF)
    c1, c2 = randn(g, 3 * C), randn(g, 3 * C)
    d1, d2 = G((M, C), BF, dev), G((M, C), BF, dev)
    K.bn_bwd_apply2(gi, y1, c1, d1.t, y2, c2, d2.t)
    for nm, d, y, co in (("dy1", d1, y1, c1), ("dy2", d2, y2, c2)):
        k1, k2, k3 = co.double().view(3, C)
        ref = k1 * gi.double() + k2 * y.double() + k3
        mag = (k1 * gi.double()).abs() + (k2 * y.double()).abs() + k3.abs()
        check("bn_bwd_apply2", dev, d.t, ref, bf16_bound(ref, mag), nm)
        d.check(nm)


test_bn_bwd_apply2_grid_stride = grid_stride(test_bn_bwd_apply2, 4096)


# ---------------------------------------------------------------------------------------------
# bn_finalize, bn_bwd_coeff, bn_eval_coeff
# ---------------------------------------------------------------------------------------------
def _fwd_slab(g, C, nshard, count):
    """A [nshard, 2, C] slab whose shard sums give mean ~ N(0, 1), var in [0.5, 2]."""
    mean, var = randn(g, C).double(), rand(g, C, lo=0.5, hi=2.0).double()
    w = rand(g, nshard, 1, C, lo=0.5, hi=1.5).double()
    w = w / w.sum(0, keepdim=True)
    tot = torch.stack([mean * count, (var + mean * mean) * count])  # [2, C]
    return (w * tot[None]).reshape(-1).contiguous()


FIN_CASES = [pytest.param(C, nsh, id=f"C{C}-nshard{nsh}") for C in (8, 64, 2048) for nsh in (1, 4, 32)]


@pytest.mark.parametrize("count", [2, 4096])
@pytest.mark.parametrize("C,nshard", FIN_CASES)
@devices
def test_bn_finalize(dev, C, nshard, count):
    g = gen(dev, 6)
    eps = f32(1e-5)
    for affine, momentum in itertools.product((True, False), (0.0, 0.1)):
        stats = _fwd_slab(g, C, nshard, count)
        gamma, beta = (randn(g, C), randn(g, C)) if affine else (None, None)
        rm0, rv0 = randn(g, C), rand(g, C, lo=0.5, hi=2.0)
        rm, rv = G(C, F32, dev, init=rm0), G(C, F32, dev, init=rv0)
        outs = [G(C, F32, dev) for _ in range(4)]
        sc, sh, mean_o, inv_o = outs
        K.bn_finalize(stats, count, gamma, beta, 1e-5, momentum, rm.t, rv.t, sc.t, sh.t, mean_o.t, inv_o.t)
        st = stats.view(nshard, 2, C).sum(0)
        mean = st[0] / count
        var = (st[1] / count - mean * mean).clamp_min(0)
        inv = 1.0 / torch.sqrt(var + eps)
        gd = gamma.double() if affine else torch.ones_like(mean)
        bd = beta.double() if affine else torch.zeros_like(mean)
        what = f"affine{int(affine)} mom{momentum}"
        check("bn_finalize", dev, sc.t, gd * inv, f32_bound((gd * inv).abs()), what + " scale")
        check("bn_finalize", dev, sh.t, bd - mean * gd * inv, f32_bound(bd.abs() + (mean * gd * inv).abs()), what + " shift")
        check("bn_finalize", dev, mean_o.t, mean, f32_bound(mean.abs()), what + " mean")
        check("bn_finalize", dev, inv_o.t, inv, f32_bound(inv.abs()), what + " invstd")
        if momentum == 0.0:  # running statistics untouched
            assert torch.equal(rm.t, rm0) and torch.equal(rv.t, rv0), what
        else:
            m = f32(momentum)
            unb = var * count / (count - 1)
            check("bn_finalize", dev, rm.t, (1 - m) * rm0.double() + m * mean,
                  f32_bound(((1 - m) * rm0.double()).abs() + (m * mean).abs()), what + " running_mean")
            check("bn_finalize", dev, rv.t, (1 - m) * rv0.double() + m * unb,
                  f32_bound(((1 - m) * rv0.double()).abs() + (m * unb).abs()), what + " running_var")
        for o in outs + [rm, rv]:
            o.check(what)
    # the outputs that may be absent
    sc, sh = G(C, F32, dev), G(C, F32, dev)
    K.bn_finalize(stats, count, None, None, 1e-5, 0.1, None, None, sc.t, sh.t, None, None)
    check("bn_finalize", dev, sc.t, inv, f32_bound(inv.abs()), "bare scale")
    check("bn_finalize", dev, sh.t, -mean * inv, f32_bound((mean * inv).abs()), "bare shift")


@pytest.mark.parametrize("count", [2, 4096])
@pytest.mark.parametrize("C,nshard", FIN_CASES)
@devices
def test_bn_bwd_coeff(dev, C, nshard, count):
    g = gen(dev, 7)
    for affine, accumulate in itertools.product((True, False), (False, True)):
        stats = randn(g, nshard * 2 * C, scale=count / nshard).double()
        gamma = randn(g, C) if affine else None
        mu, inv = randn(g, C), rand(g, C, lo=0.5, hi=2.0)
        dg0, db0 = randn(g, C), randn(g, C)
        co = G(3 * C, F32, dev)
        dg = G(C, F32, dev, init=dg0 if accumulate else None)
        db = G(C, F32, dev, init=db0 if accumulate else None)
        K.bn_bwd_coeff(stats, count, gamma, mu, inv, co.t, dg.t, db.t, accumulate=accumulate)
        st = stats.view(nshard, 2, C).sum(0)
        s, q = st[0], st[1]
        gd = gamma.double() if affine else torch.ones_like(s)
        i, m = inv.double(), mu.double()
        k1, k2 = gd * i, -gd * i * i * (q / count)
        k3a, k3b = -gd * i * (s / count), gd * i * i * (q / count) * m
        ref = torch.cat([k1, k2, k3a + k3b])
        mag = torch.cat([k1.abs(), k2.abs(), k3a.abs() + k3b.abs()])
        what = f"affine{int(affine)} acc{int(accumulate)}"
        check("bn_bwd_coeff", dev, co.t, ref, f32_bound(mag), what + " coeff")
        a = dg0.double() if accumulate else 0.0
        b = db0.double() if accumulate else 0.0
        check("bn_bwd_coeff", dev, dg.t, q + a, f32_bound(q.abs() + abs(a)), what + " dgamma")
        check("bn_bwd_coeff", dev, db.t, s + b, f32_bound(s.abs() + abs(b)), what + " dbeta")
        for o in (co, dg, db):
            o.check(what)
    co = G(3 * C, F32, dev)  # without the parameter gradients
    K.bn_bwd_coeff(stats, count, gamma, mu, inv, co.t)
    check("bn_bwd_coeff", dev, co.t, ref, f32_bound(mag), "coeff only")
    co.check()


@pytest.mark.parametrize("C", [8, 10, 64, 2048])
@devices
def test_bn_eval_coeff(dev, C):
    g = gen(dev, 8)
    eps = f32(1e-5)
    for affine in (True, False):
        gamma, beta = (randn(g, C), randn(g, C)) if affine else (None, None)
        rm, rv = randn(g, C), rand(g, C, lo=0.01, hi=4.0)
        sc, sh = G(C, F32, dev), G(C, F32, dev)
        K.bn_eval_coeff(gamma, beta, 1e-5, rm, rv, sc.t, sh.t)
        inv = 1.0 / torch.sqrt(rv.double() + eps)
        gd = gamma.double() if affine else torch.ones_like(inv)
        bd = beta.double() if affine else torch.zeros_like(inv)
        check("bn_eval_coeff", dev, sc.t, gd * inv, f32_bound((gd * inv).abs()), f"affine{int(affine)} scale")
        check("bn_eval_coeff", dev, sh.t, bd - rm.double() * gd * inv,
              f32_bound(bd.abs() + (rm.double() * gd * inv).abs()), f"affine{int(affine)} shift")
        sc.check()
        sh.check()


@devices
def test_33_shards_raise(dev):
    C = 8
    stats = torch.zeros(33 * 2 * C, dtype=F64, device=dev)
    v = lambda n=C: torch.ones(n, device=dev)  # noqa: E731
    with pytest.raises(ValueError):
        K.bn_finalize(stats, 4.0, None, None, 1e-5, 0.1, v(), v(), v(), v(), v(), v())
    with pytest.raises(ValueError):
        K.bn_bwd_coeff(stats, 4.0, None, v(), v(), v(3 * C))


# ---------------------------------------------------------------------------------------------
# max pool
# ---------------------------------------------------------------------------------------------
def _windows(t, K_, stride, pad, P, Q, fill):
    """[N, P, Q, K*K, C] window taps of the NHWC tensor ``t`` in (r, s) order; ``fill`` outside the image."""
    N, H, W, C = t.shape
    tp = torch.full((N, H + 2 * pad + K_, W + 2 * pad + K_, C), fill, dtype=t.dtype, device=t.device)
    tp[:, pad:pad + H, pad:pad + W] = t
    taps = [tp[:, r:r + stride * (P - 1) + 1:stride, s:s + stride * (Q - 1) + 1:stride]
            for r in range(K_) for s in range(K_)]
    return torch.stack(taps, 3)


def _first_max(win):
    """(max, index of its first occurrence in tap order, gap to the runner-up) over dim 3."""
    best = win.max(3).values
    nk = win.shape[3]
    idx = torch.arange(nk, device=win.device).view(1, 1, 1, nk, 1).expand_as(win)
    first = torch.where(win == best.unsqueeze(3), idx, torch.full_like(idx, nk)).min(3).values
    rest = torch.where(idx == first.unsqueeze(3), torch.full_like(win, -math.inf), win).max(3).values
    return best, first, best - rest


def _pool_out(H, K_, stride, pad):
    return (H + 2 * pad - K_) // stride + 1


def _check_maxpool_fwd(dev, x, K_, stride, pad, affine, relu, key):
    N, H, W, C = x.shape
    P, Q = _pool_out(H, K_, stride, pad), _pool_out(W, K_, stride, pad)
    g = gen(dev, 9)
    s, h = (randn(g, C), randn(g, C)) if affine else (None, None)
    out, arg, ymax = G((N, P, Q, C), BF, dev), G((N, P, Q, C), torch.uint8, dev), G((N, P, Q, C), BF, dev)
    K.maxpool_fwd(x, out.t, arg.t, K=K_, stride=stride, pad=pad, scale=s, shift=h, relu=relu, ymax=ymax.t)
    x64 = x.double()
    v = x64 * s.double() + h.double() if affine else x64
    mag = (x64 * s.double()).abs() + h.double().abs() if affine else x64.abs()
    if relu:
        v = v.clamp_min(0)
    win = _windows(v, K_, stride, pad, P, Q, -math.inf)
    wmag = _windows(mag, K_, stride, pad, P, Q, 0.0).max(3).values
    best, first, gap = _first_max(win)
    what = f"K{K_}s{stride}p{pad} affine{int(affine)} relu{int(relu)}"
    assert int(arg.t.max()) < K_ * K_, what
    if affine:
        check(key, dev, out.t, best, bf16_bound(best, wmag), what)
        sure = gap > U_CHAIN * wmag  # the float64 maximum is unique beyond fp32 rounding
        assert torch.equal(arg.t[sure], first.to(torch.uint8)[sure]), what
    else:  # exact values: a pure move, ties to the first tap in (r, s) order
        assert torch.equal(out.t, best.to(BF)), what
        assert torch.equal(arg.t, first.to(torch.uint8)), what
    # ymax: the raw input at the tap the kernel chose (a pure move)
    raw = _windows(x, K_, stride, pad, P, Q, 0.0).gather(3, arg.t.long().unsqueeze(3)).squeeze(3)
    assert torch.equal(ymax.t, raw), what
    # ... which is a tap inside the image whose value is the maximum the kernel stored
    inside = _windows(torch.ones_like(x), K_, stride, pad, P, Q, 0.0).gather(3, arg.t.long().unsqueeze(3)).squeeze(3)
    assert bool((inside == 1).all()), what
    for o in (out, arg, ymax):
        o.check(what)
    # without ymax
    out2, arg2 = G((N, P, Q, C), BF, dev), G((N, P, Q, C), torch.uint8, dev)
    K.maxpool_fwd(x, out2.t, arg2.t, K=K_, stride=stride, pad=pad, scale=s, shift=h, relu=relu)
    assert torch.equal(out2.t, out.t) and torch.equal(arg2.t, arg.t), what
    out2.check(what)
    arg2.check(what)


@pytest.mark.parametrize("C,M", row_cases())
@devices
def test_maxpool_fwd_rows(dev, C, M):
    """The row mapping of the pool: M output pixels (N = M images of 2 x 2 -> 1 x 1), on the
    constant-window path (3, 2, 1) and the generic one (2, 2, 0)."""
    x = randn(gen(dev, 10), M, 2, 2, C, dtype=BF)
    big = M > 4096
    for K_, stride, pad in ((3, 2, 1), (2, 2, 0)):
        for affine, relu in ((True, True),) if big else ((False, False), (False, True), (True, True), (True, False)):
            _check_maxpool_fwd(dev, x, K_, stride, pad, affine, relu, "maxpool_fwd_rows")


test_maxpool_fwd_rows_grid_stride = grid_stride(test_maxpool_fwd_rows, 4096)


POOL_GEOM = [(3, 2, 1), (2, 2, 0), (3, 1, 1)]
POOL_CASES = [pytest.param(k, s, p, H, W, C, id=f"K{k}s{s}p{p}-{H}x{W}-C{C}")
              for (k, s, p) in POOL_GEOM for (H, W) in ((1, 1), (2, 3), (15, 13)) for C in (8, 64)
              if (H, W) != (1, 1) or (k, s, p) == (3, 2, 1)]


@pytest.mark.parametrize("K_,stride,pad,H,W,C", POOL_CASES)
@devices
def test_maxpool_fwd(dev, K_, stride, pad, H, W, C):
    x = randn(gen(dev, 11), 2, H, W, C, dtype=BF)
    for affine, relu in ((False, False), (False, True), (True, True), (True, False)):
        _check_maxpool_fwd(dev, x, K_, stride, pad, affine, relu, "maxpool_fwd")


@pytest.mark.parametrize("K_,stride,pad,H,W,C", POOL_CASES)
@devices
def test_maxpool_bwd(dev, K_, stride, pad, H, W, C):
    N = 2
    P, Q = _pool_out(H, K_, stride, pad), _pool_out(W, K_, stride, pad)
    g = gen(dev, 12)
    x = randn(g, N, H, W, C, dtype=BF).double()
    dout = randn(g, N, P, Q, C, dtype=BF)
    # the argmax comes from the float64 oracle (first maximum in tap order): no ties to blur the comparison
    _, first, _ = _first_max(_windows(x, K_, stride, pad, P, Q, -math.inf))
    arg = first.to(torch.uint8)
    dx = G((N, H, W, C), BF, dev)
    K.maxpool_bwd(dout, arg, dx.t, K=K_, stride=stride, pad=pad)
    ref = torch.zeros(N, H + 2 * pad + K_, W + 2 * pad + K_, C, dtype=F64, device=dev)
    mag = torch.zeros_like(ref)
    for r in range(K_):
        for s in range(K_):
            c = torch.where(first == r * K_ + s, dout.double(), torch.zeros_like(dout, dtype=F64))
            ref[:, r:r + stride * (P - 1) + 1:stride, s:s + stride * (Q - 1) + 1:stride] += c
            mag[:, r:r + stride * (P - 1) + 1:stride, s:s + stride * (Q - 1) + 1:stride] += c.abs()
    ref, mag = ref[:, pad:pad + H, pad:pad + W], mag[:, pad:pad + H, pad:pad + W]
    check("maxpool_bwd", dev, dx.t, ref, U_BF16 * ref.abs() + sum_bound(K_ * K_, mag))
    dx.check()


@devices
@pytest.mark.parametrize("K_,stride,pad,H,W,C", [c for c in POOL_CASES if c.values[0] != 3 or c.values[1] != 1])
def test_pool_bn_bwd(dev, K_, stride, pad, H, W, C):
    """The stem BN backward with the max-pool backward folded in: g = maxpool_bwd(dpool) masked by
    y*scale + shift > 0; reduce: [sum g, sum g*xhat]; apply: dy = k1*g + k2*y + k3."""
    N = 2
    P, Q = _pool_out(H, K_, stride, pad), _pool_out(W, K_, stride, pad)
    g = gen(dev, 22)
    y, dpool = randn(g, N, H, W, C, dtype=BF), randn(g, N, P, Q, C, dtype=BF)
    s, h, mu, inv, co = randn(g, C), randn(g, C), randn(g, C), rand(g, C, lo=0.5, hi=2.0), randn(g, 3 * C)
    t = y.double() * s.double() + h.double()
    amb = t.abs() <= U_CHAIN * ((y.double() * s.double()).abs() + h.double().abs())
    _, first, _ = _first_max(_windows(t.clamp_min(0), K_, stride, pad, P, Q, -math.inf))
    arg = first.to(torch.uint8)
    gp = torch.zeros(N, H + 2 * pad + K_, W + 2 * pad + K_, C, dtype=F64, device=dev)
    gpm = torch.zeros_like(gp)
    for r in range(K_):
        for q in range(K_):
            c = torch.where(first == r * K_ + q, dpool.double(), torch.zeros_like(dpool, dtype=F64))
            gp[:, r:r + stride * (P - 1) + 1:stride, q:q + stride * (Q - 1) + 1:stride] += c
            gpm[:, r:r + stride * (P - 1) + 1:stride, q:q + stride * (Q - 1) + 1:stride] += c.abs()
    gp, gpm = gp[:, pad:pad + H, pad:pad + W], gpm[:, pad:pad + H, pad:pad + W]
    gm, gmm = gp * (t > 0), gpm * (t > 0)
    xhat = (y.double() - mu.double()) * inv.double()
    M, nwin = N * H * W, 4  # at most 2 x 2 windows hold a pixel
    st = _slab(C, dev)
    K.pool_bn_bwd_reduce(dpool, arg, y, s, h, mu, inv, st.t, K=K_, stride=stride, pad=pad)
    got = st.t.view(NSH, 2, C).sum(0)
    red = lambda v: v.reshape(-1, C).sum(0)  # noqa: E731
    check("pool_bn_bwd_reduce", dev, got[0], red(gm), sum_bound(M * nwin, red(gmm)) + red(gpm * amb), "sum g")
    check("pool_bn_bwd_reduce", dev, got[1], red(gm * xhat), sum_bound(M * nwin, red(gmm * xhat.abs()))
          + red(gpm * xhat.abs() * amb), "sum g*xhat")
    st.check()
    dy = G((N, H, W, C), BF, dev)
    K.pool_bn_bwd_apply(dpool, arg, y, s, h, co, dy.t, K=K_, stride=stride, pad=pad)
    k1, k2, k3 = co.double().view(3, C)
    ref = k1 * gm + k2 * y.double() + k3
    if amb.any():  # either mask value is right where fp32 rounding decides it
        alt = k1 * (gp - gm) + k2 * y.double() + k3
        ref = torch.where(amb & ((dy.t.double() - alt).abs() < (dy.t.double() - ref).abs()), alt, ref)
    mag = (k1.abs() * gpm) + (k2 * y.double()).abs() + k3.abs()
    check("pool_bn_bwd_apply", dev, dy.t, ref, bf16_bound(ref, mag) + k1.abs() * sum_bound(nwin, gpm))
    dy.check()


# ---------------------------------------------------------------------------------------------
# average pool
# ---------------------------------------------------------------------------------------------
AVG_CASES = [pytest.param(N, HW, C, id=f"N{N}-HW{HW}-C{C}") for N in (1, 3) for HW in (1, 49) for C in (8, 512, 2048)]


@pytest.mark.parametrize("N,HW,C", AVG_CASES)
@devices
def test_avgpool(dev, N, HW, C):
    H = W = math.isqrt(HW)
    g = gen(dev, 13)
    x, dout = randn(g, N, H, W, C, dtype=BF), randn(g, N, C, dtype=BF)
    out = G((N, C), BF, dev)
    K.avgpool_fwd(x, out.t)
    ref = x.double().sum((1, 2)) / HW
    mag = x.double().abs().sum((1, 2)) / HW
    check("avgpool_fwd", dev, out.t, ref, U_BF16 * ref.abs() + sum_bound(HW, mag))
    out.check()
    dx = G((N, H, W, C), BF, dev)
    K.avgpool_bwd(dout, dx.t)
    ref = (dout.double() / HW)[:, None, None, :].expand(N, H, W, C)
    check("avgpool_bwd", dev, dx.t, ref, bf16_bound(ref, ref.abs()))
    dx.check()


# ---------------------------------------------------------------------------------------------
# softmax cross-entropy
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("C", [10, 200, 257, 1000])
@devices
def test_softmax_ce(dev, C, B, dtype):
    g = gen(dev, 14)
    x = randn(g, B, C, scale=2.0)
    # row 0: an exact tie for the maximum -- the lower index wins, as in torch.argmax
    lo, hi = 3, C - 2
    x[0, lo] = x[0, hi] = float(x[0].max()) + 1.0
    x = x.to(dtype)
    labels = torch.randint(0, C, (B,), generator=g, device=dev)
    labels[0] = lo
    if B > 1:  # a second tie whose label is the higher index: not correct
        x[1, lo] = x[1, hi] = float(x[1].float().max()) + 1.0
        labels[1] = hi
    labels2 = torch.randint(0, C, (B,), generator=g, device=dev)
    lam = torch.tensor([0.3], device=dev)
    x64 = x.double()
    mx = x64.max(1, keepdim=True).values
    idx = torch.arange(C, device=dev).expand(B, C)
    amax = torch.where(x64 == mx, idx, torch.full_like(idx, C)).min(1).values
    correct = float((amax == labels).sum())
    assert correct == (1.0 if B == 1 else float((amax[2:] == labels[2:]).sum()) + 1.0)
    lse = mx.squeeze(1) + torch.log(torch.exp(x64 - mx).sum(1))
    p = torch.exp(x64 - lse[:, None])
    lo_exp = (2 + 1.16 * (x64 - mx).abs().max(1).values) * 2.0 ** -23  # fast-exponential error of the lse's terms
    for smoothing, gs, mix, outs in itertools.product((0.0, 0.1), (1.0, 0.25), (False, True), (True, False)):
        if not outs and (smoothing, gs) != (0.1, 0.25):
            continue
        sm, lm = f32(smoothing), (f32(0.3) if mix else 1.0)
        l2 = labels2 if mix else labels
        xl, xl2 = x64.gather(1, labels[:, None]).squeeze(1), x64.gather(1, l2[:, None]).squeeze(1)
        sx = x64.sum(1) / C
        loss = (1 - sm) * (lm * (lse - xl) + (1 - lm) * (lse - xl2)) + sm * (lse - sx)
        lmag = (1 - sm) * (lm * (lse.abs() + xl.abs()) + (1 - lm) * (lse.abs() + xl2.abs())) \
            + sm * (lse.abs() + x64.abs().sum(1) / C)
        lbound = f32_bound(lmag)
        t = torch.full_like(p, sm / C)
        t.scatter_add_(1, labels[:, None], torch.full((B, 1), (1 - sm) * lm, dtype=F64, device=dev))
        t.scatter_add_(1, l2[:, None], torch.full((B, 1), (1 - sm) * (1 - lm), dtype=F64, device=dev))
        inv = f32(gs) / B
        dref = (p - t) * inv
        # widened for __expf (module docstring): (2 + 1.16 |x - lse|) ulp of p, plus the lse's own error (relative, of p)
        pexp = ((2 + 1.16 * (x64 - lse[:, None]).abs()) * 2.0 ** -23 + (C * 2.0 ** -24 + U_CHAIN)
                + lo_exp[:, None]) * p * inv
        dmag = (p + t) * inv
        dplain = bf16_bound(dref, dmag) if dtype == BF else f32_bound(dmag)
        dbound = dplain + pexp
        what = f"smooth{smoothing} gs{gs} mix{int(mix)} outs{int(outs)}"
        dl = G((B, C), dtype, dev) if outs else None
        lo_ = G(B, F32, dev) if outs else None
        st0 = torch.tensor([3.5, 2.0], dtype=F64, device=dev)
        st = G(2, F64, dev, init=st0)
        K.softmax_ce(x, labels, dlogits=dl.t if outs else None, loss_out=lo_.t if outs else None, stats=st.t,
                     smoothing=smoothing, grad_scale=gs, labels2=labels2 if mix else None, lam=lam if mix else None)
        assert float(st.t[1]) == 2.0 + correct, what  # the counter adds to what was there, exactly
        check("softmax_ce", dev, st.t[0:1] - 3.5, loss.sum().reshape(1), lbound.sum().reshape(1) + 2.0 ** -50 * 3.5,
              what + " loss sum")
        st.check(what)
        if outs:
            check("softmax_ce", dev, lo_.t, loss, lbound, what + " loss")
            check("softmax_ce", dev, dl.t, dref, dbound, what + " dlogits", plain=dplain)
            dl.check(what)
            lo_.check(what)
    # no statistics slab at all
    lo_ = G(B, F32, dev)
    K.softmax_ce(x, labels, loss_out=lo_.t, smoothing=0.1, grad_scale=0.25, labels2=labels2, lam=lam)
    check("softmax_ce", dev, lo_.t, loss, lbound, "loss only")
    lo_.check()


# ---------------------------------------------------------------------------------------------
# optimizers
# ---------------------------------------------------------------------------------------------
OPT_N = [1, 3, 4, 5, 1027]


def _opt_state(dev, n, seed):
    g = gen(dev, seed)
    return randn(g, n), randn(g, n), randn(g, n), rand(g, n, lo=0.0, hi=2.0)


@pytest.mark.parametrize("n", OPT_N)
@devices
def test_sgd_step(dev, n):
    """One step from a random state, every option combination (96 per n), against torch.optim.SGD's
    rule: d = g*gs + wd*p; buf = d on the first step, else mom*buf + (1 - damp)*d; d = d + mom*buf
    (nesterov) or buf; p -= lr*d."""
    p0, g_, v0, _ = _opt_state(dev, n, 15)
    lr, wd = 0.1, 1e-2
    flr, fwd = f32(lr), f32(wd)
    gsp = torch.tensor([0.5], device=dev)
    modes = [(True, 0.0), (False, 0.0), (False, 0.5)]
    for (nesterov, damp), mom, first, p16_on, hyper_on, gsp_on in itertools.product(
            modes, (0.0, 0.9), (True, False), (True, False), (True, False), (True, False)):
        fm, gscale = f32(mom), 0.25
        gs = gscale * (0.5 if gsp_on else 1.0)
        p, v = G(n, F32, dev, init=p0), G(n, F32, dev, init=v0)
        p16 = G(n, BF, dev) if p16_on else None
        hyper = torch.tensor([lr], device=dev) if hyper_on else None
        K.sgd_step(p.t, g_, v.t, p16.t if p16_on else None, lr=(123.0 if hyper_on else lr), momentum=mom,
                   dampening=damp, weight_decay=wd, nesterov=nesterov, first=first,
                   grad_scale_ptr=gsp if gsp_on else None, grad_scale=gscale, hyper=hyper)
        what = f"nesterov{int(nesterov)} damp{damp} mom{mom} first{int(first)} p16{int(p16_on)} hyper{int(hyper_on)} gsp{int(gsp_on)}"
        d = g_.double() * gs + fwd * p0.double()
        dmag = (g_.double() * gs).abs() + (fwd * p0.double()).abs()
        if mom != 0.0:
            if first:
                buf, bmag = d, dmag
            else:
                buf = fm * v0.double() + (1 - damp) * d
                bmag = (fm * v0.double()).abs() + (1 - damp) * dmag
            check("sgd_step", dev, v.t, buf, f32_bound(bmag), what + " buf")
            d, dmag = (d + fm * buf, dmag + fm * bmag) if nesterov else (buf, bmag)
        else:  # no momentum: the buffer is not touched
            assert torch.equal(v.t, v0), what
        ref = p0.double() - flr * d
        check("sgd_step", dev, p.t, ref, f32_bound(p0.double().abs() + flr * dmag), what + " p")
        p.check(what)
        v.check(what)
        if p16_on:  # the bf16 copy: a pure cast of the stored parameter
            assert torch.equal(p16.t, p.t.to(BF)), what
            p16.check(what)


@pytest.mark.parametrize("n", OPT_N)
@devices
def test_adam_step(dev, n):
    p0, g_, m0, v0 = _opt_state(dev, n, 16)
    lr, wd, b1, b2, eps = 1e-2, 1e-2, 0.9, 0.999, 1e-8
    flr, fwd, fb1, fb2, feps = f32(lr), f32(wd), f32(b1), f32(b2), f32(eps)
    gsp = torch.tensor([0.5], device=dev)
    for decoupled, step, hyper_on, gsp_on, p16_on in itertools.product(
            (True, False), (1, 7), (True, False), (True, False), (True, False)):
        bc1, bc2 = f32(1 - b1 ** step), f32(1 - b2 ** step)
        gscale = 0.25
        gs = gscale * (0.5 if gsp_on else 1.0)
        p, m, v = G(n, F32, dev, init=p0), G(n, F32, dev, init=m0), G(n, F32, dev, init=v0)
        p16 = G(n, BF, dev) if p16_on else None
        hyper = torch.tensor([lr, 1 - b1 ** step, 1 - b2 ** step], device=dev) if hyper_on else None
        K.adam_step(p.t, g_, m.t, v.t, p16.t if p16_on else None, lr=(123.0 if hyper_on else lr), beta1=b1, beta2=b2,
                    eps=eps, weight_decay=wd, decoupled=decoupled, step=(999 if hyper_on else step),
                    grad_scale_ptr=gsp if gsp_on else None, grad_scale=gscale, hyper=hyper)
        what = f"decoupled{int(decoupled)} step{step} hyper{int(hyper_on)} gsp{int(gsp_on)} p16{int(p16_on)}"
        gg, gmag = g_.double() * gs, (g_.double() * gs).abs()
        pp, pmag = p0.double(), p0.double().abs()
        if decoupled:
            pp, pmag = pp - flr * fwd * pp, pmag + (flr * fwd * pp).abs()
        else:
            gg, gmag = gg + fwd * pp, gmag + (fwd * pp).abs()
        mm = fb1 * m0.double() + (1 - fb1) * gg
        mmag = (fb1 * m0.double()).abs() + (1 - fb1) * gmag
        vv = fb2 * v0.double() + (1 - fb2) * gg * gg
        # (gg's own error enters squared: twice its relative size, on the magnitude gmag^2)
        vmag = (fb2 * v0.double()).abs() + 2 * (1 - fb2) * gmag * gmag
        den = torch.sqrt(vv / bc2) + feps
        upd = flr * (mm / bc1) / den
        # the update's magnitude: the numerator's terms over the denominator, plus the denominator's own
        # relative error (half of vv's through the square root) on the update
        umag = flr * (mmag / bc1) / den + upd.abs() * (1 + 0.5 * vmag / vv.clamp_min(1e-300))
        check("adam_step", dev, m.t, mm, f32_bound(mmag), what + " m")
        check("adam_step", dev, v.t, vv, f32_bound(vmag), what + " v")
        check("adam_step", dev, p.t, pp - upd, f32_bound(pmag + umag), what + " p")
        for o in (p, m, v):
            o.check(what)
        if p16_on:
            assert torch.equal(p16.t, p.t.to(BF)), what
            p16.check(what)


# ---------------------------------------------------------------------------------------------
# casts, norms
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 1027])
@devices
def test_cast_f32_bf16(dev, n):
    g = gen(dev, 17)
    x = randn(g, n, scale=3.0)
    # every other element exactly halfway between two bf16 numbers (low half 0x8000), alternately above
    # an even and an odd bf16 (bit 16 clear / set): ties must round to even, i.e. down / up
    bits = x.view(torch.int32)
    i = torch.arange(n, device=dev)
    half = torch.where(i % 4 == 0, bits & ~0x1FFFF, (bits & ~0xFFFF) | 0x10000) | 0x8000
    x = torch.where(i % 2 == 0, half, bits).view(F32).contiguous()
    if n > 4:
        x[1], x[3] = 0.0, -0.0
    y = G(n, BF, dev)
    K.cast_f32_bf16(x, y.t)
    b = x.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    want = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF  # round to nearest, ties to even, on the bits
    got = y.t.view(torch.int16).to(torch.int64) & 0xFFFF
    assert torch.equal(got, want)
    y.check()


@pytest.mark.parametrize("n", [1, 1027, (1 << 20) + 1])
@devices
def test_sumsq_clip_factor(dev, n):
    x = randn(gen(dev, 18), n)
    ss = (x.double() ** 2).sum()
    work = G(4, F32, dev, init=torch.zeros(4, device=dev))
    work.t[0:2].view(F64)[0] = 7.25
    K.sumsq_accum(x, work.t)  # adds to what is there
    got = work.t[0:2].view(F64).clone()
    check("sumsq_accum", dev, got - 7.25, ss.reshape(1), sum_bound(n, ss).reshape(1) + 2.0 ** -50 * 7.25, "sum of squares")
    assert bool(torch.isnan(work.t[2:]).logical_not().all()) and float(work.t[2:].abs().sum()) == 0.0
    K.sumsq_accum(x, work.t)
    got2 = work.t[0:2].view(F64).clone()
    check("sumsq_accum", dev, got2 - got, ss.reshape(1), sum_bound(n, ss).reshape(1) + 2.0 ** -50 * got, "second add")
    nrm = torch.sqrt(got2.double())
    for rel in (0.5, 2.0):  # the norm above and below max_norm
        max_norm = float(nrm) * rel
        work.t[2:].fill_(float("nan"))
        K.clip_factor(work.t, max_norm)
        fm = f32(max_norm)
        want = torch.clamp(fm / (nrm + f32(1e-6)), max=1.0)
        check("clip_factor", dev, work.t[2:3], want, f32_bound(want.abs()), f"factor, max_norm = {rel} |g|")
        check("clip_factor", dev, work.t[3:4], nrm, f32_bound(nrm.abs()), "norm")
        if rel > 1:
            assert float(work.t[2]) == 1.0
        assert torch.equal(work.t[0:2].view(F64), got2)
    work.check()
    # the one-call form zeroes first
    work.t[0:2].view(F64)[0] = 7.25
    K.global_norm_clip_factor(x, float(torch.sqrt(ss)) * 0.5, work.t)
    check("clip_factor", dev, work.t[0:2].view(F64), ss.reshape(1), sum_bound(n, ss).reshape(1), "global_norm sumsq")
    want = torch.clamp(f32(float(torch.sqrt(ss)) * 0.5) / (torch.sqrt(work.t[0:2].view(F64).double()) + f32(1e-6)), max=1.0)
    check("clip_factor", dev, work.t[2:3], want, f32_bound(want.abs()), "global_norm factor")
    work.check()


# ---------------------------------------------------------------------------------------------
# input pipeline
# ---------------------------------------------------------------------------------------------
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _norm_ref(v255, dev):
    """((v/255 - mean)/std, magnitude) of a [..., 3] float64 tensor of 0..255 values."""
    m = torch.tensor([f32(v) for v in MEAN], dtype=F64, device=dev)
    s = torch.tensor([f32(v) for v in STD], dtype=F64, device=dev)
    return (v255 / 255.0 - m) / s, (v255 / 255.0 + m) / s


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("W", [1, 5])
@pytest.mark.parametrize("Cin", [1, 3])
@devices
def test_normalize_u8(dev, Cin, W, flip):
    N, H = 3, 2
    g = gen(dev, 19)
    img = torch.randint(0, 256, (N, H, W, Cin), generator=g, device=dev, dtype=torch.uint8)
    fl = torch.tensor([1, 0, 1], dtype=torch.uint8, device=dev) if flip else None
    out = G((N, H, W, 4), BF, dev)
    K.normalize_u8(img, out.t, MEAN, STD, flip=fl)
    src = img.double().expand(N, H, W, 3)
    if flip:
        src = torch.where(fl.bool()[:, None, None, None], src.flip(2), src)
    ref, mag = _norm_ref(src, dev)
    check("normalize_u8", dev, out.t[..., :3], ref, bf16_bound(ref, mag))
    assert torch.equal(out.t[..., 3], torch.zeros(N, H, W, dtype=BF, device=dev))  # the pad channel: exactly 0
    out.check()


def _augment_ref(img, boxes, flip, Ho, Wo):
    """float64 bilinear crop-resize (pixel-centre convention, edge clamp) of uint8 NHWC, 0..255."""
    N, Hin, Win, Cin = img.shape
    dev = img.device
    oy = torch.arange(Ho, device=dev, dtype=F64)
    ox = torch.arange(Wo, device=dev, dtype=F64)
    res = torch.zeros(N, Ho, Wo, 3, dtype=F64, device=dev)
    for n in range(N):
        by, bx, bh, bw = (float(v) for v in boxes[n])
        oxx = (Wo - 1 - ox) if (flip is not None and int(flip[n])) else ox
        sy = (by + (oy + 0.5) * bh / Ho - 0.5).clamp(0, Hin - 1)
        sx = (bx + (oxx + 0.5) * bw / Wo - 0.5).clamp(0, Win - 1)
        y0, x0 = sy.floor().long(), sx.floor().long()
        y1, x1 = (y0 + 1).clamp(max=Hin - 1), (x0 + 1).clamp(max=Win - 1)
        wy, wx = (sy - y0)[:, None, None], (sx - x0)[None, :, None]
        im = img[n].double().expand(Hin, Win, 3)
        res[n] = ((im[y0][:, x0] * (1 - wx) + im[y0][:, x1] * wx) * (1 - wy)
                  + (im[y1][:, x0] * (1 - wx) + im[y1][:, x1] * wx) * wy)
    return res


# Boxes (y0, x0, h, w): sizes Ho (Wo) times a power of two and origins on multiples of 1/4, so every
# source coordinate and bilinear weight is exact in fp32 (no floor() can flip between fp32 and float64)
# and the per-element bound applies to the interpolation; boxes 0 and 2 reach past the image (edge clamp).
AUG_CASES = [
    pytest.param(37, 3, 9, [(-1.25, -2.5, 16, 16), (0.75, 3.25, 8, 32), (2.0, 30.25, 4, 16)], id="W37-C3"),
    pytest.param(30, 1, 9, [(-1.25, -2.5, 16, 16), (0.75, 3.25, 8, 16), (2.0, 20.25, 4, 16)], id="W30-C1"),
    pytest.param(1400, 3, 5, [(-0.5, 300.25, 4, 1024), (0.25, -8.0, 8, 2048), (1.0, 1390.5, 4, 16)], id="W1400-C3"),
]
# 96-byte rows from a 16-byte aligned base: the two source rows go through LDS
AUG_STAGED = pytest.param(32, 3, 9, [(-1.25, -2.5, 16, 16), (0.75, 3.25, 8, 16), (2.0, 14.25, 4, 16)], id="W32-C3-staged")


@pytest.mark.parametrize("cutmix", [False, True])
@pytest.mark.parametrize("Win,Cin,Hin,boxes", AUG_CASES + [AUG_STAGED])
@devices
def test_augment_u8(dev, Win, Cin, Hin, boxes, cutmix):
    """The non-staged path (rows whose byte length is no multiple of 16, or longer than 4096 bytes) and the
    staged one (with cutmix: both passes of a row reuse the staged rows), with flips, and a CutMix box that
    touches the top and right image edges."""
    N, Ho, Wo = 3, 8, 8
    g = gen(dev, 20)
    img = torch.randint(0, 256, (N, Hin, Win, Cin), generator=g, device=dev, dtype=torch.uint8)
    bx = torch.tensor(boxes, dtype=F32, device=dev)
    fl = torch.tensor([0, 1, 1], dtype=torch.uint8, device=dev)
    perm = torch.tensor([2, 0, 1], dtype=torch.int32, device=dev) if cutmix else None
    mixbox = torch.tensor([0, 5, 3, Wo], dtype=torch.int32, device=dev) if cutmix else None
    out = G((N, Ho, Wo, 4), BF, dev)
    K.augment_u8(img, out.t, bx, MEAN, STD, flip=fl, perm=perm, mixbox=mixbox)
    v = _augment_ref(img, bx, fl, Ho, Wo)
    if cutmix:
        pasted = v.clone()
        pasted[:, 0:5, 3:Wo] = v[perm.long()][:, 0:5, 3:Wo]
        v = pasted
    ref, mag = _norm_ref(v, dev)
    check("augment_u8", dev, out.t[..., :3], ref, bf16_bound(ref, mag))
    assert torch.equal(out.t[..., 3], torch.zeros(N, Ho, Wo, dtype=BF, device=dev))
    out.check()


# ---------------------------------------------------------------------------------------------
# weight_prep
# ---------------------------------------------------------------------------------------------
WP_TR = [(64, 1, 64), (128, 9, 64), (192, 1, 64), (512, 9, 512)]  # the last: 576 tiles > the 512 blocks
WP_CAST = [1, 3, 5, 10, 700, 1000 * 2048]
WP_STEM = [(64, 7, 7, 3), (64, 3, 3, 3), (16, 7, 7, 1)]
WP_ZERO = [1, 2, 7, 4097]
WP_COUNT = [1, 20, 300]


def _al(v, a):
    return (v + a - 1) // a * a


@devices
def test_weight_prep(dev):
    """One launch over a shuffled list of all entry kinds, from the fp32 master and again from a bf16
    source of the same layout. The whole destination buffer is compared bit for bit with a buffer that
    holds the sentinel wherever nothing may be written (stem padding: exactly zero)."""
    g = gen(dev, 21)
    entries = [("tr", e) for e in WP_TR] + [("cast", n) for n in WP_CAST] + [("stem", e) for e in WP_STEM]
    if dev != "cpu":  # the absolute-pointer kinds exist on the GPU only
        entries += [("zero", k) for k in WP_ZERO] + [("count", k) for k in WP_COUNT]
    order = torch.randperm(len(entries), generator=torch.Generator().manual_seed(5)).tolist()
    entries = [entries[i] for i in order]
    # layout: sources on multiples of 16 elements, destinations on multiples of 64 (the program's
    # alignment), GUARD sentinel elements between neighbours
    src_off = dst_off = GUARD
    zoff, coff = 2, 1
    plan = []
    for kind, e in entries:
        if kind == "tr":
            n = e[0] * e[1] * e[2]
            plan.append((kind, e, src_off, dst_off, _al(dst_off + n + GUARD, 64)))
            dst_off = _al(dst_off + n + GUARD, 64) + n
        elif kind == "cast":
            n = e
            plan.append((kind, e, src_off, dst_off, None))
            dst_off += n
        elif kind == "stem":
            n = e[0] * e[1] * e[2] * e[3]
            plan.append((kind, e, src_off, dst_off, None))
            dst_off += e[0] * 256
        elif kind == "zero":
            plan.append((kind, e, zoff, None, None))
            zoff = _al(zoff + e + 2, 2)
            continue
        else:
            plan.append((kind, e, coff, None, None))
            coff += e + 1
            continue
        src_off = _al(src_off + n + GUARD, 16)
        dst_off = _al(dst_off + GUARD, 64)
    master = randn(g, src_off, scale=0.1)
    zbuf = torch.full((zoff + 2,), float("nan"), dtype=F64, device=dev)
    zbits = zbuf.view(torch.int64)
    zbits.fill_(_SENTINEL[F64])
    cbuf0 = torch.randint(0, 1000, (coff + 1,), generator=g, device=dev, dtype=torch.int64)
    descs, want = [], torch.full((dst_off,), _SENTINEL[BF], dtype=torch.int16, device=dev)
    want_bf = want.view(BF)
    zwant, cwant = zbits.clone(), cbuf0.clone()
    for kind, e, so, do, to in plan:
        if kind == "tr":
            Kc, RS, Cc = e
            n = Kc * RS * Cc
            descs.append((so, do, to, Kc, RS, Cc))
            w = master[so:so + n].to(BF)
            want_bf[do:do + n] = w
            want_bf[to:to + n] = w.view(Kc, RS, Cc).permute(2, 1, 0).reshape(-1)  # CRSK
        elif kind == "cast":
            descs.append((so, do, -1, e, 1, 1))
            want_bf[do:do + e] = master[so:so + e].to(BF)
        elif kind == "stem":
            Kc, R, S, Cc = e
            descs.append((so, do, -2, Kc, R * 16 + S, Cc))
            o = torch.zeros(Kc, 8, 8, 4, dtype=BF, device=dev)
            o[:, :R, :S, :Cc] = master[so:so + Kc * R * S * Cc].view(Kc, R, S, Cc).to(BF)
            want_bf[do:do + Kc * 256] = o.reshape(-1)
        elif kind == "zero":
            descs.append((zbuf.data_ptr() + 8 * so, 0, -3, e, 0, 0))
            zbuf[so:so + e] = float("nan")
            zwant[so:so + e] = 0
        else:
            descs.append((None, 0, -4, e, 0, 0))  # (the address: of the run's own counter buffer)
            cwant[so:so + e] += 1
    assert len(descs) == len(entries)
    zstart = zbuf.clone()
    for source in (master, master.to(BF)):
        wbuf = torch.empty(dst_off, dtype=BF, device=dev)
        wbuf.view(torch.int16).fill_(_SENTINEL[BF])
        zbuf.copy_(zstart)
        cbuf = cbuf0.clone()
        ds = [(cbuf.data_ptr() + 8 * p[2], *d[1:]) if d[0] is None else d for d, p in zip(descs, plan)]
        K.weight_prep(source, wbuf, K.pack_wdesc(ds, dev), len(ds))
        nm = str(source.dtype)
        got = wbuf.view(torch.int16)
        if not torch.equal(got, want):
            bad = (got != want).nonzero().flatten()
            raise AssertionError(f"{nm}: {bad.numel()} destination elements differ, first at {int(bad[0])}")
        assert torch.equal(zbits, zwant), f"{nm}: zeroing entries"
        assert torch.equal(cbuf, cwant), f"{nm}: counter entries"


@devices
def test_pack_wdesc_rejects_truncated_channels(dev):
    """The transposed copy is made in 64 x 64 tiles: a K or C that is no multiple of 64 would be
    silently truncated, so the descriptor builder (which ResNetProgram uses) refuses it."""
    for Kc, Cc in ((96, 64), (64, 32), (64, 100), (0, 64)):
        with pytest.raises(ValueError):
            K.pack_wdesc([(0, 0, 6144, Kc, 1, Cc)], dev)
    d = K.pack_wdesc([(0, 0, 4096, 64, 1, 64), (16, 64, -1, 10, 1, 3), (0, 0, -2, 16, 7 * 16 + 7, 1)], dev)
    assert d.dtype == torch.int32 and d.numel() == 30  # 40 bytes per entry
    assert d[:6].view(torch.int64).tolist() == [0, 0, 4096] and d[6:10].tolist() == [64, 1, 64, 0]


@devices
def test_program_rejects_truncated_channels(dev):
    """ResNetProgram builds its descriptors through pack_wdesc."""
    from dbx_distributed_pytorch_examples_amd.engine import program
    fake = SimpleNamespace(dev=torch.device(dev))
    with pytest.raises(ValueError):
        program.ResNetProgram._pack_wdesc(fake, [(0, 0, 96 * 64, 96, 1, 64)])
    assert torch.equal(program.ResNetProgram._pack_wdesc(fake, [(0, 0, 4096, 64, 1, 64)]),
                       K.pack_wdesc([(0, 0, 4096, 64, 1, 64)], dev))


# ---------------------------------------------------------------------------------------------
# dampening: the trainers refuse it
# ---------------------------------------------------------------------------------------------
@devices
def test_trainers_reject_dampening(dev):
    """The trainers step with ``first=False`` on a zeroed momentum buffer, which is torch's first-step
    rule (buf = d) only without dampening; a captured step cannot switch rules after its first replay.
    So every trainer refuses ``dampening != 0`` instead of training differently from torch.optim.SGD."""
    import torch.nn as nn
    from dbx_distributed_pytorch_examples_amd.engine.frozen_trainer import NativeHead
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig
    from dbx_distributed_pytorch_examples_amd.models import resnet18
    from dbx_distributed_pytorch_examples_amd.parallel.fsdp import ShardedDataParallel
    from dbx_distributed_pytorch_examples_amd.parallel.zero import SegmentedZero, ZeroShardedOptimizer
    d = torch.device(dev)
    bad = OptimConfig(momentum=0.9, dampening=0.5)
    with pytest.raises(ValueError, match="dampening"):
        NativeTrainer(resnet18(num_classes=10), 2, (32, 32), d, optim=bad, use_graphs=False)
    with pytest.raises(ValueError, match="dampening"):
        NativeHead(nn.Linear(8, 4), 2, d, bad)
    z = torch.zeros(16, device=d)
    with pytest.raises(ValueError, match="dampening"):
        ZeroShardedOptimizer(z, z.clone(), bad)
    with pytest.raises(ValueError, match="dampening"):
        SegmentedZero(None, bad, [], [])
    with pytest.raises(ValueError, match="dampening"):
        ShardedDataParallel(nn.Linear(8, 4).to(d), bad)
    # and without dampening the first trainer step is torch's: buf = d (undamped), so mom / grad == 1
    ok = OptimConfig(lr=0.1, momentum=0.9, dampening=0.0, weight_decay=0.0)
    ZeroShardedOptimizer(z, z.clone(), ok)
    p0 = torch.tensor([1.0, -2.0, 3.0, 0.5], device=d)
    gr = torch.tensor([0.5, 0.25, -1.0, 2.0], device=d)
    p, v = p0.clone(), torch.zeros(4, device=d)
    K.sgd_step(p, gr, v, None, lr=0.1, momentum=0.9, dampening=0.0, first=False)  # the trainers' call
    tp = torch.nn.Parameter(p0.clone())
    opt = torch.optim.SGD([tp], lr=0.1, momentum=0.9, dampening=0.0)
    tp.grad = gr.clone()
    opt.step()
    assert torch.equal(v, opt.state[tp]["momentum_buffer"]) and torch.equal(p, tp.detach())


@devices
def test_autograd_engine_passes_dampening(dev):
    from dbx_distributed_pytorch_examples_amd.engine.autograd_trainer import build_torch_optimizer
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import OptimConfig
    tp = torch.nn.Parameter(torch.zeros(2, device=dev))
    opt = build_torch_optimizer([tp], OptimConfig(momentum=0.9, dampening=0.5))
    assert opt.param_groups[0]["dampening"] == 0.5
    assert build_torch_optimizer([tp], OptimConfig()).param_groups[0]["dampening"] == 0.0
