"""Per-element checks of the matrix-core convolutions (csrc/conv_igemm_kernel.h, conv_fast.hip, conv_sweep.hip,
conv_patch3.hip, conv_group.hip, stem_bwd.hip) through ``ops.kernels``, every kernel and option forced by ``tile=`` /
``dma=`` / ``rounds=`` / ``cnt=`` and the engine switches ``splitk_wgs`` / ``tap_prune``.

Every test runs on the CPU (``ops.kernels`` dispatches CPU tensors to ``ops/reference.py``: the test's own logic and
data are checked without a GPU, and the reference path is pinned) and on the GPU (the HIP kernels). The oracle is plain
float64 torch written here -- one matrix product per filter tap -- on the CPU tensors; never ``reference.py``, never
``F.conv2d``, never another kernel.

Two data legs per kernel:

* ``exact``: small-integer operands (activations / gradients in -2..2, weights in {-1, 0, 1} with at most ``nnz``
  non-zeros per reduction row, BN scales in {1, 2}, shifts / means in {-1, 0, 1}, inverse deviations and backward
  coefficients powers of two; the fp32 weight gradients dense in -3..3). Every product, every partial sum in any
  order and every stored value is then exactly representable, so outputs and statistics must equal the float64
  oracle bit for bit. The test asserts on the oracle alone, before any kernel output is looked at, that every bf16
  result is a multiple of 0.5 of magnitude <= 128 and every fp32 result at most 2^22.
* ``rand``: ``randn`` operands at the scaling of the older conv tests, per element
  ``|got - ref| <= 2^-8 |ref| + (K 2^-24 + 2^-21) sum|term|`` (bf16 outputs; fp32 outputs the second term only; K the
  reduction length, sum|term| the float64 sum of the absolute products). On top, only what the operation itself
  defines: an operand the kernel rounds to bf16 from an fp32 chain (BN prologue, tail, folded BN backward) may land on
  the neighbouring bf16 value where the float64 value lies within the chain's 2^-20 error of a rounding tie -- those
  elements (found from the oracle) add their one-ulp difference times |w|; a data gradient with an addend or epilogue
  with an addend is rounded to bf16 twice (tile, then tile + addend); a mask whose float64 argument is within the chain
  error of zero may fall either way. Statistics: ``sum_bound`` over the rows plus the summed element bounds. Each of
  these is a widening of the plain formula; its plain ratio is recorded and reported below.

Every output (``out``, ``dx``, ``dw``, ``tail_out``, ``tail_bits``, ``act_out``, ``dy_out``, the statistics slabs) and the
weight-gradient workspace lives in a guarded allocation: sentinel elements on both sides that must be unchanged,
the body NaN (or a known base in the accumulate modes) that must come back finite.

The largest ``err / bound`` of each random-leg test is collected in ``RATIOS`` (printed at the end of the module; written
as JSON to ``$DBX_CONV_ELEM_RATIOS`` when set). A widened bound (``widened``) also records its ratio against the plain
formula, under "<test>, bound not widened" (not asserted). Measured on an MI355X: every exact case bit-equal, and

* bf16 outputs: at most 0.996 of their bound in every forward and data-gradient test (the rounding of the stored value
  alone reaches 2^-8 |ref|; the CPU leg gives the same figures); fp32 weight gradients: conv_wgrad 0.066, stem 0.028,
  patch 0.002, grouped inside "group conv" 0.994 -- the matrix cores stay inside 2^-24 per addition at these lengths;
* widened for the tie slack of a bf16 operand (BN prologue, tail, fold), cause above: plain ratio at most 0.991
  (conv_fwd pro1 0.984, tail 0.991, sweep fwd 0.991, patch fwd pro1 0.956, fold plain 0.983, sweep dgrad plain 0.988,
  conv_wgrad pro1 0.062) -- the hardware did not need it on this data;
* widened for a MASK_Y argument within the chain error of zero (the element may be masked either way; likewise an
  ambiguous ``tail_bits`` bit is not compared): plain ratio at most 0.981 (mask_y 0.964, fold mask_y 0.981, fast 0.980,
  patch 0.918) -- not needed on this data;
* widened for the second bf16 rounding of a data gradient with an addend (``accumulate`` / ``addsrc``: the tile is
  rounded, the addend added in fp32, the sum rounded again, so the error scales with |tile|, not |ref|): needed, plain
  ratio 59.5 (accum / add1), 27.0 (add2), 92.6 (tiny accum), 105.8 (fold add1), 57.6 (fast), 126.0 (sweep add1);
  a mask-only epilogue rounds nothing again and keeps the plain bound (mask_out+bn2 0.961);
* statistics, widened by the summed element bounds because they are sums of the STORED bf16 values: needed, plain
  ratio up to 9191 (forward, "... stats") and 920 (data gradients); against the widened bound 0.801 and 0.302.

``relu_in=False`` exists only without a BN prologue (the kernels refuse a prologue without ReLU), where it must change
nothing: the plain-operand calls pass it.
"""
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

from dbx_distributed_pytorch_examples_amd.ops import kernels as K

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
devices = pytest.mark.parametrize("dev", DEVICES)
legs = pytest.mark.parametrize("leg", ["exact", "rand"])

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U_BF16 = 2.0 ** -8     # bf16 unit roundoff
U_CHAIN = 2.0 ** -20   # 16 fp32 roundings of an elementwise chain
RATIOS = {}
NSH = 4                # statistics shards of the tests' slabs


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    if not RATIOS:
        return
    print("\n[test_conv_elem] largest err / bound per test and device:")
    for k in sorted(RATIOS):
        print(f"  {k}: {RATIOS[k]:.4f}")
    path = os.environ.get("DBX_CONV_ELEM_RATIOS")
    if path:
        with open(path, "w") as f:
            json.dump(RATIOS, f, indent=1, sort_keys=True)


# ---------------------------------------------------------------------------------------------
# helpers (Guarded / check / sum_bound as in test_nn_ops.py; the comparisons run on the CPU, next to the oracle)
# ---------------------------------------------------------------------------------------------
def sum_coef(n):
    """``sum_bound`` of test_nn_ops.py as a factor of sum|term|: n fp32 terms in any summation order."""
    return n * 2.0 ** -24 + 2.0 ** -21


def _where(ratio, shape):
    i = int(ratio.flatten().argmax())
    return i, tuple(int(v) for v in torch.unravel_index(torch.tensor(i), shape))


def widened(plain, extra):
    """``plain + extra``: a bound widened by a term with a stated cause. The issue's plain formula rides along, so that
    ``check`` records the ratio against it too (not asserted): it shows whether the widening was needed."""
    b = plain + extra
    b.plain = plain
    return b


def check(key, dev, got, ref, bound, what):
    """Every element of ``got`` is finite and within ``bound`` of the float64 ``ref``; records the largest err / bound, and
    for a ``widened`` bound also the largest err / plain bound."""
    got = got.detach().cpu().double().reshape(ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite (unwritten?) output elements"
    err = (got - ref).abs()
    plain = getattr(bound, "plain", None)
    if plain is not None:
        r = torch.where(err == 0, torch.zeros_like(err), err / plain.reshape(ref.shape))
        k = f"{key}[{dev}], bound not widened"
        RATIOS[k] = max(RATIOS.get(k, 0.0), float(r.max()))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    k = f"{key}[{dev}]"
    RATIOS[k] = max(RATIOS.get(k, 0.0), worst)
    if not worst <= 1.0:
        i, idx = _where(ratio, ref.shape)
        raise AssertionError(f"{what}: element {idx}: got {got.flatten()[i].item()!r}, want {ref.flatten()[i].item()!r}, "
                             f"err {err.flatten()[i].item():.3e} > bound {bound.flatten()[i].item():.3e} "
                             f"(ratio {worst:.3f}; {int((ratio > 1).sum())} of {ratio.numel()} elements out)")


def exact(got, ref, what):
    """Bit-equality with the float64 oracle, element by element."""
    got = got.detach().cpu().double().reshape(ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite (unwritten?) output elements"
    if not torch.equal(got, ref):
        bad = got != ref
        i, idx = _where(bad.double(), ref.shape)
        raise AssertionError(f"{what}: element {idx}: got {got.flatten()[i].item()!r}, want {ref.flatten()[i].item()!r} "
                             f"({int(bad.sum())} of {ref.numel()} elements differ; first rows "
                             f"{sorted(set(bad.reshape(-1, ref.shape[-1]).any(1).nonzero().flatten().tolist()))[:8]})")


def verify(leg, key, dev, got, ref, bound, what):
    if leg == "exact":
        exact(got, ref, what)
    else:
        check(key, dev, got, ref, bound, what)


def pre_bf16(ref, what):
    """Condition of the exact leg, on the oracle alone: bf16 stores a multiple of 0.5 of magnitude <= 128 exactly."""
    assert bool(((ref * 2).round() == ref * 2).all()) and float(ref.abs().max()) <= 128, f"{what}: oracle not bf16-exact"


def pre_f32(ref, what):
    """fp32 holds a multiple of 0.25 of magnitude <= 2^22 exactly (g * xhat of the folded gradients has quarters)."""
    assert bool(((ref * 4).round() == ref * 4).all()) and float(ref.abs().max()) <= 2 ** 22, f"{what}: oracle not fp32-exact"


_INT = {BF: torch.int16, F32: torch.int32, F64: torch.int64, torch.uint8: torch.uint8}
_SENTINEL = {BF: 0x7FA5, F32: 0x7FC0A5A5, F64: 0x7FF8A5A5A5A5A5A5, torch.uint8: 0xA5}
GUARD = 64  # elements on each side (a multiple of 16 bytes for every dtype: the body keeps its alignment)


class Guarded:
    """A tensor ``t`` of ``shape`` in the middle of a larger allocation whose guard elements hold a sentinel bit
    pattern. ``t`` starts as NaN (floats) / 0xFF (bytes), or as a copy of ``init``."""

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
        else:
            self.t.fill_(float("nan"))

    def check(self, what=""):
        g = torch.cat([self.bits[:GUARD], self.bits[GUARD + self.n:]])
        assert bool((g == _SENTINEL[self.dtype]).all()), f"{what}: wrote outside the output region"


def new_stats(C, dev):
    return Guarded(NSH * 2 * C, F64, dev, init=torch.zeros(NSH * 2 * C, dtype=F64))


def stats_total(st, C):
    return st.t.detach().cpu().view(-1, 2, C).sum(0)


def gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def ints(g, shape, lo, hi, dtype=BF):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).to(dtype)


def randn(g, shape, dtype=BF, scale=1.0):
    return (torch.randn(tuple(shape), generator=g) * scale).to(dtype)


def choice(g, n, values, dtype=F32):
    v = torch.tensor(values, dtype=dtype)
    return v[torch.randint(0, len(values), (n,), generator=g)]


def sparse_w(g, rows, cols, nnz):
    """[rows, cols] bf16 in {-1, 0, 1}: at most ``nnz`` non-zeros per row, at positions drawn per row. With few rows of a
    long reduction some positions stay zero in every row (about 40 % at 64 rows of 1728): every tap and channel block
    is still hit many times, and the rand leg's dense weights cover each single position."""
    w = torch.zeros(rows, cols)
    n = min(nnz, cols)
    idx = torch.rand(rows, cols, generator=g).argsort(1)[:, :n]
    w.scatter_(1, idx, (torch.randint(0, 2, (rows, n), generator=g) * 2 - 1).float())
    return w.to(BF)


def weights(leg, g, rows, cols, nnz=24):
    return sparse_w(g, rows, cols, nnz) if leg == "exact" else randn(g, (rows, cols), scale=1 / math.sqrt(cols))


def acts(leg, g, shape):
    return ints(g, shape, -2, 2) if leg == "exact" else randn(g, shape)


def pack_bits(mask):
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.int32)
    return (mask.reshape(-1, 8).to(torch.int32) * w).sum(1).to(torch.uint8)


def bf16_operand(a64, mag):
    """The bf16 value of an operand that a kernel computes by an fp32 chain (exact value ``a64``, sum of the absolute
    terms ``mag``) and its ``slack``: 0 where every fp32 value within the chain's error rounds to the same bf16 value,
    else the distance to the neighbouring bf16 value it may round to."""
    win = U_CHAIN * mag
    r = a64.float().bfloat16().double()
    _, e = torch.frexp(a64.abs().clamp_min(1e-300))
    ulp = torch.ldexp(torch.ones_like(a64), e - 8)
    near = (ulp / 2 - (a64 - r).abs()) <= win
    slack = torch.where(a64.abs() <= 2 * win, 2 * win, torch.where(near, ulp, torch.zeros_like(a64)))
    return r, slack


# ---------------------------------------------------------------------------------------------
# the float64 oracle: one matrix product per filter tap
# ---------------------------------------------------------------------------------------------
def out_hw(H, W, R, S, st, pad):
    return (H + 2 * pad - R) // st + 1, (W + 2 * pad - S) // st + 1


def _padded(x, pad):
    return F.pad(x, (0, 0, pad, pad, pad, pad))


def conv64(x, w, st, pad):
    """x [N, H, W, IC], w [OC, R, S, IC] (float64) -> [N, OH, OW, OC]."""
    OC, R, S, _ = w.shape
    OH, OW = out_hw(x.shape[1], x.shape[2], R, S, st, pad)
    xp = _padded(x, pad)
    out = torch.zeros(x.shape[0], OH, OW, OC, dtype=F64)
    for r in range(R):
        for s in range(S):
            out += xp[:, r:r + (OH - 1) * st + 1:st, s:s + (OW - 1) * st + 1:st] @ w[:, r, s].t()
    return out


def dgrad64(dy, w, H, W, st, pad):
    """dy [N, P, Q, K], w [K, R, S, C] (float64) -> dx [N, H, W, C]."""
    Kc, R, S, C = w.shape
    N, P, Q, _ = dy.shape
    dxp = torch.zeros(N, H + 2 * pad, W + 2 * pad, C, dtype=F64)
    for r in range(R):
        for s in range(S):
            dxp[:, r:r + (P - 1) * st + 1:st, s:s + (Q - 1) * st + 1:st] += dy @ w[:, r, s]
    return dxp[:, pad:pad + H, pad:pad + W].contiguous()


def wgrad64(dy, x, R, S, st, pad):
    """dy [N, P, Q, K], x [N, H, W, C] (float64) -> dw [K, R, S, C]."""
    N, P, Q, Kc = dy.shape
    xp = _padded(x, pad)
    dw = torch.zeros(Kc, R, S, x.shape[-1], dtype=F64)
    d2 = dy.reshape(-1, Kc)
    for r in range(R):
        for s in range(S):
            dw[:, r, s] = d2.t() @ xp[:, r:r + (P - 1) * st + 1:st, s:s + (Q - 1) * st + 1:st].reshape(d2.shape[0], -1)
    return dw


def bn_pro(leg, g, IC):
    if leg == "exact":
        return choice(g, IC, [1.0, 2.0]), choice(g, IC, [-1.0, 0.0, 1.0])
    return torch.rand(IC, generator=g) + 0.5, torch.randn(IC, generator=g) * 0.1


def pro64(x, sc, sh, res=None, rsc=None, rsh=None):
    """relu(x * sc + sh [+ res [* rsc + rsh]]) in float64, the sum of its absolute terms, and the pre-ReLU value."""
    t = x.double() * sc.double() + sh.double()
    mag = (x.double() * sc.double()).abs() + sh.double().abs()
    if res is not None:
        r = res.double()
        if rsc is not None:
            mag = mag + (r * rsc.double()).abs() + rsh.double().abs()
            r = r * rsc.double() + rsh.double()
        else:
            mag = mag + r.abs()
        t = t + r
    return t.clamp_min(0), mag, t


def fwd_stats_ref(leg, ref, b):
    """[sum y, sum y^2] over the rows of the stored outputs and their bounds (rand leg: the stored y is within b of ref)."""
    OC = ref.shape[-1]
    y = ref.reshape(-1, OC)
    tot = torch.stack([y.sum(0), (y * y).sum(0)])
    if leg == "exact":
        pre_f32(tot, "statistics")
        return tot, None
    b = b.reshape(-1, OC)
    M = y.shape[0]
    hi = y.abs() + b
    # plain: sum_bound over the rows of the oracle's terms. Widened: the statistics are those of the STORED outputs,
    # each within b of the oracle (and y^2 is one more fp32 rounding)
    plain = sum_coef(M) * torch.stack([y.abs().sum(0), (y * y).sum(0)])
    b0 = b.sum(0) + sum_coef(M) * hi.sum(0)
    b1 = (2 * y.abs() * b + b * b).sum(0) + (sum_coef(M) + U_CHAIN) * (hi * hi).sum(0)
    return tot, widened(plain, torch.stack([b0, b1]) - plain)


def check_fwd_stats(leg, key, dev, st, OC, tot, tb, what):
    verify(leg, key + " stats", dev, stats_total(st, OC), tot, tb, what + " statistics")
    st.check(what + " statistics")


# ---------------------------------------------------------------------------------------------
# implicit-GEMM forward
# ---------------------------------------------------------------------------------------------
FWD_TILES = [(64, 64), (128, 64), (128, 128), (256, 64), (256, 128), (128, 256)]
FWD_CASES = [
    # N, H, W, IC, OC, R, stride, pad
    (1, 5, 7, 64, 64, 1, 1, 0),      # M = 35 < every bm: one partial tile; 1 K block; H != W, both odd
    (3, 13, 11, 192, 192, 1, 1, 0),  # M = 429: tile rows straddle the images (143 rows each); 3 K blocks; OC = 3 * 64
    (2, 13, 11, 64, 128, 3, 1, 1),   # M = 286: two 256-row tiles, the last partial; 9 K blocks; halo on odd 13 x 11
    (3, 5, 7, 128, 256, 3, 1, 1),    # 18 K blocks: the default split-K engages; OC = 256 = bn of (128, 256)
    (1, 9, 7, 192, 64, 3, 2, 1),     # stride 2 on odd sizes; 27 K blocks (odd count of the 32-channel stages x 2)
    (2, 14, 14, 64, 384, 3, 2, 1),   # stride 2 on an even size; OC = 3 * 128
]
TINY_CASES = [(4, h, w, 64, 64, 3, st, 1) for (h, w) in ((1, 1), (1, 2), (2, 2)) for st in (1, 2)]  # pruned taps


def _id(c):
    return "x".join(str(v) for v in c)


def fwd_problem(leg, seed, case, pro, nnz=24):
    N, H, W, IC, OC, R, st, pad = case
    g = gen(seed)
    x = acts(leg, g, (N, H, W, IC))
    w = weights(leg, g, OC, R * R * IC, nnz)
    sc = sh = None
    a, slack = x.double(), None
    if pro:
        sc, sh = bn_pro(leg, g, IC)
        a64, mag, _ = pro64(x, sc, sh)
        a, slack = bf16_operand(a64, mag)
    w64 = w.double().view(OC, R, R, IC)
    ref = conv64(a, w64, st, pad)
    b = None
    if leg == "exact":
        pre_bf16(ref, "out")
    else:
        b = U_BF16 * ref.abs() + sum_coef(R * R * IC) * conv64(a.abs(), w64.abs(), st, pad)
        if pro:  # widened: the prologue's operand may round to the neighbouring bf16 value near a tie
            b = widened(b, conv64(slack, w64.abs(), st, pad))
    return x, w, sc, sh, ref, b


def run_fwd(key, dev, leg, case, pro, combos, engine):
    """Every combo with statistics; the first one also without."""
    N, H, W, IC, OC, R, st, pad = case
    x, w, sc, sh, ref, b = fwd_problem(leg, 11, case, pro)
    tot, tb = fwd_stats_ref(leg, ref, b)
    xd, wd = x.to(dev), w.to(dev)
    scd, shd = (None, None) if sc is None else (sc.to(dev), sh.to(dev))
    for i, (tile, sk, prune) in enumerate(combos if dev == "cuda" else combos[:1]):
        engine(splitk_wgs=sk, tap_prune=prune)
        for with_stats in ((True, False) if i == 0 else (True,)):
            what = f"conv_fwd {_id(case)} pro{int(pro)} tile{tile} splitk_wgs={sk} tap_prune={prune} stats{int(with_stats)}"
            out = Guarded(ref.shape, BF, dev)
            stt = new_stats(OC, dev) if with_stats else None
            K.conv_fwd(xd, wd, out.t, R=R, S=R, stride=st, pad=pad, stats=stt.t if with_stats else None, in_scale=scd,
                       in_shift=shd, relu_in=pro, tile=tile)
            verify(leg, key, dev, out.t, ref, b, what)
            out.check(what)
            if with_stats:
                check_fwd_stats(leg, key, dev, stt, OC, tot, tb, what)


def fwd_combos(case, pro):
    """(tile with dma, splitk_wgs, tap_prune): every tile that divides OC on every operand path of its kind; the
    launches of >= 16 K blocks on the split-capable paths (dma 0 / 1) with the split-K at its default and off."""
    N, H, W, IC, OC, R, st, pad = case
    out = []
    for bm, bn in FWD_TILES:
        if OC % bn:
            continue
        for dma in ((0, 1) if pro else (0, 2, 3, 6)):
            out.append(((bm, bn, dma), None, None))
            if R * R * (IC // 64) >= 16 and dma in (0, 1):
                out.append(((bm, bn, dma), 0, None))
    return out


@legs
@pytest.mark.parametrize("pro", [False, True])
@pytest.mark.parametrize("case", FWD_CASES, ids=_id)
@devices
def test_conv_fwd(dev, case, pro, leg, engine):
    run_fwd(f"conv_fwd pro{int(pro)}", dev, leg, case, pro, fwd_combos(case, pro), engine)


@legs
@pytest.mark.parametrize("pro", [False, True])
@pytest.mark.parametrize("case", TINY_CASES, ids=_id)
@devices
def test_conv_fwd_tiny_maps(dev, case, pro, leg, engine):
    """1x1, 1x2 and 2x2 inputs under a 3x3 pad-1 filter: the launch visits only the taps that touch data (fwd_taps),
    or all of them with ``tap_prune`` off -- the same result either way."""
    combos = [((bm, 64, dma), None, prune) for prune in (None, False) for bm in (64, 128)
              for dma in ((0, 1) if pro else (0, 2, 6))]
    run_fwd(f"conv_fwd tiny pro{int(pro)}", dev, leg, case, pro, combos, engine)


@legs
@devices
def test_conv_fwd_uneven_splitk(dev, leg, engine):
    """17 K blocks (IC = 1088 at 1x1, past the prologue's channel limit: plain operands): the default split-K cuts them
    into slices of 9 and 8 -- every other case here splits evenly."""
    combos = [((bm, 64, 0), sk, None) for bm in (64, 128, 256) for sk in (None, 0)]
    run_fwd("conv_fwd uneven split-K", dev, leg, (1, 5, 7, 1088, 64, 1, 1, 0), False, combos, engine)


TAIL_CASES = [(1, 5, 7, 64, 64), (3, 13, 11, 128, 256)]  # N, H, W, IC, OC (1x1): one partial tile; straddling rows


@legs
@pytest.mark.parametrize("res_bn", [False, True])
@pytest.mark.parametrize("case", TAIL_CASES, ids=_id)
@devices
def test_conv_fwd_tail(dev, case, res_bn, leg):
    """Tail prologue: act = relu(x * scale + shift + r), r = tail_res or tail_res * rs + rh, stored to ``tail_out`` with
    its 1-bit mask in ``tail_bits`` and consumed by the 1x1 conv."""
    N, H, W, IC, OC = case
    g = gen(12)
    x, res = acts(leg, g, (N, H, W, IC)), acts(leg, g, (N, H, W, IC))
    w = weights(leg, g, OC, IC, nnz=12)  # act reaches 2 * 2 + 1 + 2 * 2 + 1 = 10: 12 * 10 <= 128
    sc, sh = bn_pro(leg, g, IC)
    rsc, rsh = bn_pro(leg, g, IC) if res_bn else (None, None)
    a64, mag, t = pro64(x, sc, sh, res, rsc, rsh)
    a, slack = bf16_operand(a64, mag)
    w64 = w.double().view(OC, 1, 1, IC)
    ref = conv64(a, w64, 1, 0)
    sure = t.abs() > U_CHAIN * mag  # elsewhere the mask bit may fall either way
    ab = b = None
    if leg == "exact":
        pre_bf16(ref, "out")
        pre_bf16(a64, "tail_out")
    else:
        ab = U_BF16 * a64.abs() + U_CHAIN * mag
        b = widened(U_BF16 * ref.abs() + sum_coef(IC) * conv64(a.abs(), w64.abs(), 1, 0), conv64(slack, w64.abs(), 1, 0))
    tot, tb = fwd_stats_ref(leg, ref, b)
    d = lambda v: None if v is None else v.to(dev)  # noqa: E731
    combos = [(bm, bn, dma) for bm, bn in FWD_TILES if OC % bn == 0 for dma in (0, 1)]
    for tile in combos if dev == "cuda" else combos[:1]:
        what = f"tail {_id(case)} res_bn{int(res_bn)} tile{tile}"
        out, tout, tbits, stt = Guarded(ref.shape, BF, dev), Guarded(x.shape, BF, dev), Guarded(x.numel() // 8, torch.uint8, dev), new_stats(OC, dev)
        K.conv_fwd(d(x), d(w), out.t, R=1, S=1, stride=1, pad=0, stats=stt.t, in_scale=d(sc), in_shift=d(sh), tile=tile,
                   tail_res=d(res), tail_res_scale=d(rsc), tail_res_shift=d(rsh), tail_out=tout.t, tail_bits=tbits.t)
        key = f"conv_fwd tail res_bn{int(res_bn)}"
        verify(leg, key, dev, out.t, ref, b, what + " out")
        verify(leg, key, dev, tout.t, a64, ab, what + " tail_out")
        bits = tbits.t.cpu()
        assert torch.equal(bits, pack_bits(tout.t.cpu().float() > 0)), what + ": tail_bits are not the mask of tail_out"
        want = pack_bits(t > 0)
        amb = pack_bits(~sure) if leg == "rand" else torch.zeros_like(want)
        assert torch.equal(bits | amb, want | amb), what + " tail_bits"
        for o in (out, tout, tbits):
            o.check(what)
        check_fwd_stats(leg, key, dev, stt, OC, tot, tb, what)


# ---------------------------------------------------------------------------------------------
# data gradients
# ---------------------------------------------------------------------------------------------
def dgrad_problem(leg, seed, case, variant, fold):
    """One data-gradient problem and its float64 answers. ``variant``: '+'-joined subset of accum (dx += on a base),
    add1 / add2 (addsrc at full / half resolution), mask_out, mask_y (with act_out), bn2 (second BN statistic)."""
    N, H, W, C, Kc, R, st, pad = case
    P, Q = out_hw(H, W, R, R, st, pad)
    v = set(variant.split("+")) - {"plain"}
    g = gen(seed)
    p = dict(v=v)
    p["dy"] = dy = acts(leg, g, (N, P, Q, Kc))
    p["wt"] = wt = weights(leg, g, C, R * R * Kc)  # CRSK: row c is the reduction of input channel c
    w64 = wt.double().view(C, R, R, Kc).permute(3, 1, 2, 0)  # [K, R, S, C]
    op, slack = dy.double(), None
    if fold:  # the operand is the BN-backward apply k1 * g + k2 * y + k3, rounded to bf16 (and stored to dy_out)
        p["yb"] = yb = acts(leg, g, (N, P, Q, Kc))
        if leg == "exact":
            co = torch.stack([choice(g, Kc, [0.5, 1.0]), choice(g, Kc, [-0.5, 0.5]), choice(g, Kc, [-1.0, 0.0, 1.0])])
        else:
            co = torch.randn(3, Kc, generator=g) * 0.5
        p["coeff"] = co
        k = co.double()
        op64 = k[0] * dy.double() + k[1] * yb.double() + k[2]
        omag = (k[0] * dy.double()).abs() + (k[1] * yb.double()).abs() + k[2].abs()
        op, slack = bf16_operand(op64, omag)
        p["dy_out"], p["dy_out_b"] = op64, U_BF16 * op64.abs() + U_CHAIN * omag
        if leg == "exact":
            pre_bf16(op64, "dy_out")
    c = dgrad64(op, w64, H, W, st, pad)
    b1 = None
    if leg == "rand":
        b1 = U_BF16 * c.abs() + sum_coef(R * R * Kc) * dgrad64(op.abs(), w64.abs(), H, W, st, pad)
        if fold:
            b1 = b1 + dgrad64(slack, w64.abs(), H, W, st, pad)
    ref = c
    if "accum" in v:
        p["base"] = base = acts(leg, g, (N, H, W, C))
        ref = ref + base.double()
    for sub in (1, 2):
        if f"add{sub}" in v:
            add = acts(leg, g, (N, H // sub, W // sub, C))
            p["addsrc"], p["add_sub"] = add, sub
            full = torch.zeros(N, H, W, C, dtype=F64)
            full[:, ::sub, ::sub] = add.double()
            ref = ref + full
    b = b1
    if leg == "rand" and v & {"accum", "add1", "add2"}:  # the tile is rounded to bf16, then tile + addend again
        b = b1 * (1 + U_BF16) + U_BF16 * ref.abs()
    if "mask_out" in v or "mask_y" in v:
        p["ybn"] = ybn = acts(leg, g, (N, H, W, C))
        if leg == "exact":
            mean, inv = choice(g, C, [-1.0, 0.0, 1.0]), choice(g, C, [0.5, 1.0, 2.0])
        else:
            mean, inv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
        p["mean"], p["inv"] = mean, inv
        if "mask_out" in v:
            mask = torch.rand(N, H, W, C, generator=g) > 0.5
            p["mbits"] = pack_bits(mask)
        else:
            p["sc"], p["sh"] = sc, sh = bn_pro(leg, g, C)
            a64, amag, t = pro64(ybn, sc, sh)
            mask = t > 0
            p["act"], p["act_b"] = a64, U_BF16 * a64.abs() + U_CHAIN * amag
            if leg == "exact":
                pre_bf16(a64, "act_out")
            else:
                b = b + torch.where(t.abs() <= U_CHAIN * amag, ref.abs(), torch.zeros_like(ref))
        ref = ref * mask

        def moments(y, mean, inv):
            xh = (y.double() - mean.double()) * inv.double()
            gm = ref.reshape(-1, C)
            tot = torch.stack([gm.sum(0), (gm * xh.reshape(-1, C)).sum(0)])
            if leg == "exact":
                pre_f32(tot, "statistics")
                return tot, None
            bb, ax = b.reshape(-1, C), xh.abs().reshape(-1, C)
            hi = gm.abs() + bb
            M = gm.shape[0]
            xe = ((y.double().abs() + mean.double().abs()) * inv.double()).reshape(-1, C)  # fp32 rounding of xhat
            plain = sum_coef(M) * torch.stack([gm.abs().sum(0), (gm.abs() * ax).sum(0)])  # widened: stored g, fp32 xhat
            wide = torch.stack([bb.sum(0) + sum_coef(M) * hi.sum(0),
                                (bb * ax).sum(0) + sum_coef(M) * (hi * ax).sum(0) + U_CHAIN * (hi * xe).sum(0)])
            return tot, widened(plain, wide - plain)
        p["st1"] = moments(ybn, mean, inv)
        if "bn2" in v:
            p["ybn2"] = ybn2 = acts(leg, g, (N, H, W, C))
            if leg == "exact":
                p["mean2"], p["inv2"] = choice(g, C, [-1.0, 0.0, 1.0]), choice(g, C, [0.5, 1.0, 2.0])
            else:
                p["mean2"], p["inv2"] = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
            p["st2"] = moments(ybn2, p["mean2"], p["inv2"])
    if leg == "exact":
        pre_bf16(ref, "dx")
    if leg == "rand":  # the issue's formula on the result; whatever b holds beyond it is one of the widenings above
        plain = U_BF16 * ref.abs() + sum_coef(R * R * Kc) * dgrad64(op.abs(), w64.abs(), H, W, st, pad)
        b = b if torch.equal(b, plain) else widened(plain, b - plain)
    p["ref"], p["b"] = ref, b
    return p


def run_dgrad(key, dev, leg, case, variant, tiles, engine=None, fold=False, switches=((None, None),)):
    N, H, W, C, Kc, R, st, pad = case
    p = dgrad_problem(leg, 21, case, variant, fold)
    v = p["v"]
    d = {k: t.to(dev) for k, t in p.items() if isinstance(t, torch.Tensor) and k not in ("ref", "b")}
    combos = [(t, s) for t in tiles for s in switches]
    for tile, (sk, prune) in combos if dev == "cuda" else combos[:1]:
        if engine is not None:
            engine(splitk_wgs=sk, tap_prune=prune)
        what = f"conv_dgrad {_id(case)} {variant} fold{int(fold)} tile{tile} splitk_wgs={sk} tap_prune={prune}"
        dx = Guarded((N, H, W, C), BF, dev, init=p.get("base"))
        outs = [dx]
        kw = {}
        if fold:
            dyo = Guarded(p["dy"].shape, BF, dev)
            outs.append(dyo)
            kw.update(bwd_y=d["yb"], bwd_coeff=d["coeff"], dy_out=dyo.t)
        if "addsrc" in p:
            kw.update(addsrc=d["addsrc"], add_sub=p["add_sub"])
        if "st1" in p:
            s1 = new_stats(C, dev)
            outs.append(s1)
            ekw = {}
            if "mask_y" in v:
                act = Guarded((N, H, W, C), BF, dev)
                outs.append(act)
                ekw.update(scale=d["sc"], shift=d["sh"], act_out=act.t)
            else:
                ekw.update(mbits=d["mbits"])
            if "st2" in p:
                s2 = new_stats(C, dev)
                outs.append(s2)
                ekw.update(ybn2=d["ybn2"], mean2=d["mean2"], inv2=d["inv2"], stats2=s2.t)
            kw["epilogue"] = K.BNBwdEpilogue(K.MASK_Y if "mask_y" in v else K.MASK_OUT, d["ybn"], d["mean"], d["inv"], s1.t,
                                             **ekw)
        K.conv_dgrad(d["dy"], d["wt"], dx.t, R=R, S=R, stride=st, pad=pad, accumulate="accum" in v, tile=tile, **kw)
        verify(leg, key, dev, dx.t, p["ref"], p["b"], what + " dx")
        if fold:
            verify(leg, key, dev, dyo.t, p["dy_out"], p["dy_out_b"], what + " dy_out")
        if "st1" in p:
            verify(leg, key + " stats", dev, stats_total(s1, C), *p["st1"], what + " stats1")
            if "mask_y" in v:
                verify(leg, key, dev, act.t, p["act"], p["act_b"], what + " act_out")
            if "st2" in p:
                verify(leg, key + " stats", dev, stats_total(s2, C), *p["st2"], what + " stats2")
        for o in outs:
            o.check(what)


DGRAD_CASES = [
    # N, H, W, C (dx channels), K (dy channels), R, stride, pad
    (1, 5, 7, 64, 64, 1, 1, 0),      # one partial tile, 1 K block
    (3, 13, 11, 128, 192, 3, 1, 1),  # rows straddle the images, 27 K blocks (default split-K), halo on odd sizes
    (2, 9, 7, 64, 128, 3, 2, 1),     # stride 2 on odd sizes: the four phases are 5x4, 5x3, 4x4, 4x3 with 4, 2, 2, 1 taps
    (2, 14, 14, 256, 64, 3, 2, 1),   # stride 2 on an even size; a half-resolution addend fits; C = 256 for (128, 256)
]
DGRAD_TILES = [(64, 64), (128, 128), (256, 64), (128, 256), (128, 64), (256, 128)]


def dgrad_tiles(C, dmas):
    return [(bm, bn, dma) for bm, bn in DGRAD_TILES if C % bn == 0 for dma in dmas]


@legs
@pytest.mark.parametrize("variant", ["plain", "accum", "add1", "mask_out+add1", "mask_y", "mask_out+bn2", "mask_y+accum"])
@pytest.mark.parametrize("case", DGRAD_CASES, ids=_id)
@devices
def test_conv_dgrad(dev, case, variant, leg, engine):
    N, H, W, C, Kc, R, st, pad = case
    kb = (-(-R // st)) ** 2 * (Kc // 64)  # K blocks of the largest phase
    sw = ((None, None), (0, None)) if kb >= 16 else ((None, None),)
    run_dgrad(f"conv_dgrad {variant}", dev, leg, case, variant, dgrad_tiles(C, (0, 2)), engine, switches=sw)


@legs
@pytest.mark.parametrize("variant", ["add2", "mask_out+add2", "mask_y+add2"])
@devices
def test_conv_dgrad_half_res_addend(dev, variant, leg):
    run_dgrad(f"conv_dgrad {variant}", dev, leg, DGRAD_CASES[3], variant, dgrad_tiles(256, (0, 2))[::2])


@legs
@pytest.mark.parametrize("variant", ["plain", "accum"])
@pytest.mark.parametrize("case", [(4, h, w, 64, 64, 3, st, 1) for (h, w) in ((1, 1), (1, 2), (2, 2)) for st in (1, 2)]
                         + [(2, 8, 6, 128, 64, 1, 2, 0)], ids=_id)
@devices
def test_conv_dgrad_tiny_maps(dev, case, variant, leg, engine):
    """Tiny maps (dgrad_phases drops the taps that only see padding; with ``tap_prune`` off it keeps them) and the 1x1
    stride-2 gradient, three of whose four phases have no tap at all and must come back zero."""
    run_dgrad(f"conv_dgrad tiny {variant}", dev, leg, case, variant, [(64, 64, 0), (128, 64, 2)], engine,
              switches=((None, None), (None, False)))


@legs
@pytest.mark.parametrize("variant", ["plain", "mask_y", "add1", "mask_out+add1", "mask_out+bn2+add1"])
@pytest.mark.parametrize("case", [(1, 5, 7, 64, 64, 1, 1, 0), (3, 13, 11, 256, 128, 1, 1, 0)], ids=_id)
@devices
def test_conv_dgrad_folded_bn_backward(dev, case, variant, leg):
    run_dgrad(f"conv_dgrad fold {variant}", dev, leg, case, variant, dgrad_tiles(case[3], (0, 1)), fold=True)


# ---------------------------------------------------------------------------------------------
# eight-wave kernel (tile (256, bn, 5): the whole batch on csrc/conv_fast.hip)
# ---------------------------------------------------------------------------------------------
FAST_CASES = [(3, 13, 11, 128, 256, 1, 1, 0),   # M = 429: two 256-row tiles, the last partial, rows straddle images
              (2, 13, 11, 64, 768, 3, 1, 1),    # 3x3 halo; OC = 3 * 256
              (1, 5, 7, 192, 256, 3, 1, 1)]     # one partial tile, 27 K blocks


@legs
@pytest.mark.parametrize("case", FAST_CASES, ids=_id)
@devices
def test_fast_fwd(dev, case, leg, engine):
    run_fwd("fast fwd", dev, leg, case, False, [((256, bn, 5), None, None) for bn in (128, 256)], engine)


@legs
@pytest.mark.parametrize("variant", ["plain", "mask_out+add1", "mask_y", "mask_y+add1"])
@pytest.mark.parametrize("case", [(3, 13, 11, 256, 128, 1, 1, 0), (2, 13, 11, 256, 64, 3, 1, 1)], ids=_id)
@devices
def test_fast_dgrad(dev, case, variant, leg):
    tiles = [(256, 128, 5)] + ([] if "mask_y" in variant else [(256, 256, 5)])  # (MASK_Y: the 128-wide tile only)
    run_dgrad(f"fast dgrad {variant}", dev, leg, case, variant, tiles)


# ---------------------------------------------------------------------------------------------
# N-sweep kernel (tile (128, 256, 8), csrc/conv_sweep.hip)
# ---------------------------------------------------------------------------------------------
@legs
@pytest.mark.parametrize("IC,OC", [(64, 256), (128, 256), (192, 768), (256, 256)])
@devices
def test_sweep_fwd(dev, IC, OC, leg, engine):
    run_fwd("sweep fwd", dev, leg, (3, 13, 11, IC, OC, 1, 1, 0), True, [((128, 256, 8), None, None)], engine)


@legs
@pytest.mark.parametrize("variant", ["plain", "add1", "mask_out+add1", "mask_out+bn2+add1"])
@pytest.mark.parametrize("Kc,C", [(64, 256), (192, 512), (256, 256)])
@devices
def test_sweep_dgrad(dev, Kc, C, variant, leg):
    run_dgrad(f"sweep dgrad {variant}", dev, leg, (3, 13, 11, C, Kc, 1, 1, 0), variant, [(128, 256, 8)], fold=True)


# ---------------------------------------------------------------------------------------------
# 3x3 patch kernels (64 -> 64 at width 56, csrc/conv_patch3.hip)
# ---------------------------------------------------------------------------------------------
PATCH_CASES = [(1, 8, 56), (3, 16, 56)]  # one 8-row band; several bands and images


@legs
@pytest.mark.parametrize("pro", [False, True])
@pytest.mark.parametrize("nhw", PATCH_CASES, ids=_id)
@devices
def test_patch_fwd(dev, nhw, pro, leg, engine):
    run_fwd(f"patch fwd pro{int(pro)}", dev, leg, (*nhw, 64, 64, 3, 1, 1), pro,
            [("patch_r", None, None), ("patch_s", None, None)], engine)


@legs
@pytest.mark.parametrize("variant", ["plain", "mask_y"])
@pytest.mark.parametrize("nhw", PATCH_CASES, ids=_id)
@devices
def test_patch_dgrad(dev, nhw, variant, leg):
    run_dgrad(f"patch dgrad {variant}", dev, leg, (*nhw, 64, 64, 3, 1, 1), variant, ["patch_r", "patch_s"])


# ---------------------------------------------------------------------------------------------
# weight gradients
# ---------------------------------------------------------------------------------------------
def wgrad_problem(leg, seed, case, pro):
    N, H, W, IC, OC, R, st, pad = case
    P, Q = out_hw(H, W, R, R, st, pad)
    g = gen(seed)
    if leg == "exact":
        x, dy = ints(g, (N, H, W, IC), -3, 3), ints(g, (N, P, Q, OC), -3, 3)
    else:
        x, dy = randn(g, (N, H, W, IC)), randn(g, (N, P, Q, OC))
    sc = sh = slack = None
    a = x.double()
    if pro:
        sc, sh = bn_pro(leg, g, IC)
        a64, mag, _ = pro64(x, sc, sh)
        a, slack = bf16_operand(a64, mag)
    ref = wgrad64(dy.double(), a, R, R, st, pad)
    b = None
    if leg == "exact":
        pre_f32(ref, "dw")
    else:
        b = sum_coef(N * P * Q) * wgrad64(dy.double().abs(), a.abs(), R, R, st, pad)
        if pro:  # widened: the prologue's operand may round to the neighbouring bf16 value near a tie
            b = widened(b, wgrad64(dy.double().abs(), slack, R, R, st, pad))
    return x, dy, sc, sh, ref, b


def rs(b, shape):
    """``b.reshape(shape)``, a ``widened`` bound staying one."""
    plain = getattr(b, "plain", None)
    return b.reshape(shape) if plain is None else widened(plain.reshape(shape), (b - plain).reshape(shape))


def acc_ref(leg, acc, ref, b, base, M):
    """The answer and bound of ``accumulate=True, scale=0.5``: 0.5 * dw + base. The scaling by a power of two is exact, so
    the base is one more term of the fp32 sum: ``sum_bound`` over M + 1 terms (any widening of ``b`` scales along)."""
    if not acc:
        return ref, b
    want = 0.5 * ref + base.double()
    if leg == "exact":
        pre_f32(want, "dw")
        return want, None
    plain = getattr(b, "plain", b)
    p2 = sum_coef(M + 1) * (0.5 * plain / sum_coef(M) + base.double().abs())
    return want, p2 if plain is b else widened(p2, 0.5 * (b - plain))


def ws_elems(M, OC, KTOT, bm, bn, rounds):
    """The workspace ``conv_wgrad`` needs at this split depth: the slabs and the reduction's level-1 partials."""
    nsplit, _ = K.wgrad_splits(M, OC, KTOT, bm, bn, 1 << 40, rounds)
    return nsplit, max(64, (nsplit + min(64, nsplit)) * OC * KTOT)


WGRAD_TILES = [(64, 64), (128, 64), (64, 128), (128, 128), (256, 128), (128, 256)]
WGRAD_CASES = [
    # N, H, W, IC, OC, R, stride, pad
    (2, 7, 5, 256, 256, 1, 1, 0),    # every tile fits; M = 70: one partial 64-pixel stage after a whole one
    (3, 21, 19, 64, 128, 3, 1, 1),   # M = 1197: three splits of 512 pixels, the last partial; halo on odd 21 x 19
    (2, 9, 7, 128, 64, 3, 2, 1),     # stride 2 on odd sizes
    (5, 31, 29, 64, 64, 1, 1, 0),    # M = 4495: nine splits, the two-level reduction
    (4, 2, 2, 64, 64, 3, 1, 1),      # a tiny map: most taps see padding only
    (2, 25, 23, 256, 256, 3, 1, 1),  # every tile at M = 1150: three splits (slabs + reduce, cnt), 18 stages a split, halo
]
DEEP = 1e6  # rounds= that gives the deepest split: 512 pixels per split


def run_wgrad(key, dev, leg, case, pro, calls, **fixed):
    """``calls``: (tile, dma, rounds, use_cnt, accumulate)."""
    N, H, W, IC, OC, R, st, pad = case
    x, dy, sc, sh, ref, b = wgrad_problem(leg, 31, case, pro)
    P, Q = dy.shape[1:3]
    KTOT = R * R * IC
    g = gen(32)
    base = ints(g, (OC, KTOT), -3, 3, F32) if leg == "exact" else randn(g, (OC, KTOT), F32)
    d = lambda v: None if v is None else v.to(dev)  # noqa: E731
    xd, dyd, scd, shd = d(x), d(dy), d(sc), d(sh)
    for tile, dma, rounds, use_cnt, acc in calls if dev == "cuda" else calls[:1]:
        what = f"conv_wgrad {_id(case)} pro{int(pro)} tile{tile} dma{dma} rounds={rounds} cnt{int(use_cnt)} acc{int(acc)}"
        nsplit, n = ws_elems(N * P * Q, OC, KTOT, *tile, rounds)
        ws = Guarded(n, F32, dev)
        dw = Guarded((OC, KTOT), F32, dev, init=base if acc else None)
        cnt = torch.zeros(K.wgrad_tiles_max(OC, KTOT), dtype=torch.int32, device=dev) if use_cnt else None
        K.conv_wgrad(dyd, xd, dw.t, ws.t, R=R, S=R, stride=st, pad=pad, in_scale=scd, in_shift=shd, tile=tile, dma=dma,
                     rounds=rounds, cnt=cnt, accumulate=acc, scale=0.5 if acc else 1.0)
        want, wb = acc_ref(leg, acc, ref.reshape(OC, KTOT), None if b is None else rs(b, (OC, KTOT)), base, N * P * Q)
        verify(leg, key, dev, dw.t, want, wb, what + f" ({nsplit} splits)")
        dw.check(what)
        ws.check(what + " workspace")


@legs
@pytest.mark.parametrize("pro", [False, True])
@pytest.mark.parametrize("case", WGRAD_CASES, ids=_id)
@devices
def test_conv_wgrad(dev, case, pro, leg):
    """Every tile on every operand path at the deepest split with the separate reduce; on the first and the last tile also one split
    (the kernel writes ``dw`` itself), the in-launch reduction (``cnt``), and ``accumulate`` with ``scale=0.5`` on each."""
    IC, OC = case[3], case[4]
    tiles = [t for t in WGRAD_TILES if OC % t[0] == 0 and IC % t[1] == 0]
    calls = [(t, dma, DEEP, False, False) for t in tiles for dma in ((-1,) if pro else (-1, 0, 2, 3))]
    for t in (tiles[0], tiles[-1]):
        calls += [(t, -1, 0, False, False), (t, -1, DEEP, True, False), (t, -1, 0, False, True),
                  (t, -1, DEEP, False, True), (t, -1, DEEP, True, True), (t, -1, None, False, False)]
    run_wgrad(f"conv_wgrad pro{int(pro)}", dev, leg, case, pro, calls)


@legs
@pytest.mark.parametrize("nhw", PATCH_CASES, ids=_id)
@devices
def test_patch_wgrad(dev, nhw, leg):
    N, H, W = nhw
    case = (N, H, W, 64, 64, 3, 1, 1)
    x, dy, _, _, ref, b = wgrad_problem(leg, 33, case, False)
    g = gen(34)
    base = ints(g, (64, 576), -3, 3, F32) if leg == "exact" else randn(g, (64, 576), F32)
    for acc in (False, True):
        what = f"conv_wgrad patch {_id(nhw)} acc{int(acc)}"
        ws = Guarded((K.num_cus() + 64) * 64 * 576, F32, dev)
        dw = Guarded((64, 576), F32, dev, init=base if acc else None)
        K.conv_wgrad(dy.to(dev), x.to(dev), dw.t, ws.t, R=3, S=3, stride=1, pad=1, tile="patch", accumulate=acc,
                     scale=0.5 if acc else 1.0)
        want, wb = acc_ref(leg, acc, ref.reshape(64, 576), None if b is None else rs(b, (64, 576)), base, N * H * W)
        verify(leg, "patch wgrad", dev, dw.t, want, wb, what)
        dw.check(what)
        ws.check(what + " workspace")


# ---------------------------------------------------------------------------------------------
# grouped 3x3 (csrc/conv_group.hip)
# ---------------------------------------------------------------------------------------------
def dense_group_w(w, C, cpg):
    """[C, 3, 3, cpg] (KRSC within the group) -> the block-diagonal dense [C, 3, 3, C]."""
    full = torch.zeros(C, 3, 3, C, dtype=F64)
    for o in range(C):
        g0 = o // cpg * cpg
        full[o, :, :, g0:g0 + cpg] = w[o]
    return full


@legs
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("nhw", [(3, 7, 5), (2, 8, 8)], ids=_id)  # odd H != W with rows straddling images; even
@pytest.mark.parametrize("cpg", K.GROUP_CPG)
@devices
def test_group_conv(dev, cpg, nhw, stride, leg):
    """Forward (with statistics), data gradient and weight gradient of the grouped conv at the smallest C each
    channels-per-group value allows."""
    N, H, W = nhw
    C = max(64, 2 * cpg)
    groups = C // cpg
    P, Q = out_hw(H, W, 3, 3, stride, 1)
    g = gen(41 + cpg)
    x, dy = acts(leg, g, (N, H, W, C)), acts(leg, g, (N, P, Q, C))
    w = weights(leg, g, C, 9 * cpg, nnz=16)  # (the data gradient reduces over the columns: 16 keeps those short too)
    wd = dense_group_w(w.double().view(C, 3, 3, cpg), C, cpg)
    key = "group conv"
    what = f"group cpg{cpg} {_id(nhw)} s{stride}"
    # forward
    ref = conv64(x.double(), wd, stride, 1)
    b = None
    if leg == "exact":
        pre_bf16(ref, "out")
    else:
        b = U_BF16 * ref.abs() + sum_coef(9 * cpg) * conv64(x.double().abs(), wd.abs(), stride, 1)
    tot, tb = fwd_stats_ref(leg, ref, b)
    out, stt = Guarded(ref.shape, BF, dev), new_stats(C, dev)
    K.group_conv_fwd(x.to(dev), w.to(dev), out.t, groups=groups, stride=stride, stats=stt.t)
    verify(leg, key, dev, out.t, ref, b, what + " fwd")
    out.check(what + " fwd")
    check_fwd_stats(leg, key, dev, stt, C, tot, tb, what)
    # data gradient
    wk = wd  # [K = out channel, R, S, C = in channel]
    ref = dgrad64(dy.double(), wk, H, W, stride, 1)
    if leg == "exact":
        pre_bf16(ref, "dx")
    else:
        b = U_BF16 * ref.abs() + sum_coef(9 * cpg) * dgrad64(dy.double().abs(), wk.abs(), H, W, stride, 1)
    dx = Guarded((N, H, W, C), BF, dev)
    K.group_conv_dgrad(dy.to(dev), w.to(dev), dx.t, groups=groups, stride=stride)
    verify(leg, key, dev, dx.t, ref, b, what + " dgrad")
    dx.check(what + " dgrad")
    # weight gradient (dense integers: fp32 output)
    if leg == "exact":
        x, dy = ints(g, x.shape, -3, 3), ints(g, dy.shape, -3, 3)
    full = wgrad64(dy.double(), x.double(), 3, 3, stride, 1)
    fullb = sum_coef(N * P * Q) * wgrad64(dy.double().abs(), x.double().abs(), 3, 3, stride, 1)
    pick = lambda t: torch.stack([t[o, :, :, o // cpg * cpg:o // cpg * cpg + cpg] for o in range(C)]).reshape(C, 9 * cpg)  # noqa: E731
    base = ints(g, (C, 9 * cpg), -3, 3, F32) if leg == "exact" else randn(g, (C, 9 * cpg), F32)
    for acc in (False, True):
        want, wb = acc_ref(leg, acc, pick(full), pick(fullb), base, N * P * Q)
        ws = Guarded(16 * C * 9 * cpg, F32, dev)
        dw = Guarded((C, 9 * cpg), F32, dev, init=base if acc else None)
        K.group_conv_wgrad(dy.to(dev), x.to(dev), dw.t, ws.t, groups=groups, stride=stride, accumulate=acc,
                           scale=0.5 if acc else 1.0)
        verify(leg, key, dev, dw.t, want, wb, what + f" wgrad acc{int(acc)}")
        dw.check(what + " wgrad")
        ws.check(what + " wgrad workspace")


# ---------------------------------------------------------------------------------------------
# stem (7x7 stride 2 on the image padded to four channels)
# ---------------------------------------------------------------------------------------------
STEM_CASES = [(2, 32, 32),   # the generic kernel (the patch kernel takes 224-wide images only)
              (1, 9, 13),    # odd H != W, which stem_patch_supported rejects: the generic kernel
              (1, 8, 224)]   # four output rows at width 224: the patch kernel when ``patch`` allows it


@legs
@pytest.mark.parametrize("nhw", STEM_CASES, ids=_id)
@devices
def test_stem(dev, nhw, leg, engine):
    N, H, W = nhw
    P, Q = out_hw(H, W, 7, 7, 2, 3)
    g = gen(51)
    x4 = torch.zeros(N, H, W, 4, dtype=BF)
    x4[..., :3] = acts(leg, g, (N, H, W, 3))
    wp = torch.zeros(64, 8, 8, 4, dtype=BF)
    wp[:, :7, :7, :3] = (sparse_w(g, 64, 147, 24) if leg == "exact" else randn(g, (64, 147), scale=0.05)).view(64, 7, 7, 3)
    w64 = wp.double()[:, :7, :7, :]
    ref = conv64(x4.double(), w64, 2, 3)
    b = None
    if leg == "exact":
        pre_bf16(ref, "out")
    else:
        b = U_BF16 * ref.abs() + sum_coef(256) * conv64(x4.double().abs(), w64.abs(), 2, 3)
    tot, tb = fwd_stats_ref(leg, ref, b)
    assert K.stem_patch_supported(H, W, 64, 7, 7, 2, 3) == (W == 224)
    for patch in (True, False):
        what = f"stem fwd {_id(nhw)} patch{int(patch)}"
        out, stt = Guarded(ref.shape, BF, dev), new_stats(64, dev)
        K.conv_stem_fwd(x4.to(dev), wp.view(64, 256).to(dev), out.t, stats=stt.t, patch=patch)
        verify(leg, "stem fwd", dev, out.t, ref, b, what)
        out.check(what)
        check_fwd_stats(leg, "stem fwd", dev, stt, 64, tot, tb, what)
    # weight gradient: the padded (64, 8, 8, 4) layout (zero in the padding taps), or the real taps into out_krsc
    dy = ints(g, (N, P, Q, 64), -3, 3) if leg == "exact" else randn(g, (N, P, Q, 64))
    if leg == "exact":
        x4[..., :3] = ints(g, (N, H, W, 3), -3, 3)
    real = wgrad64(dy.double(), x4.double(), 7, 7, 2, 3)
    realb = sum_coef(N * P * Q) * wgrad64(dy.double().abs(), x4.double().abs(), 7, 7, 2, 3) if leg == "rand" else None
    full = torch.zeros(64, 8, 8, 4, dtype=F64)
    full[:, :7, :7] = real
    fullb = None
    if leg == "rand":
        fullb = torch.zeros_like(full)
        fullb[:, :7, :7] = realb
    if leg == "exact":
        pre_f32(real, "dw")
    for mode, krsc in (("tile", False), ("tile", True), ("generic", False)):
        engine(stem_wgrad=mode)
        what = f"stem wgrad {_id(nhw)} {mode} out_krsc{int(krsc)}"
        ws, dw = Guarded(16 * 1024 * 1024, F32, dev), Guarded((64, 256), F32, dev)
        ok = Guarded((64, 7, 7, 3), F32, dev) if krsc else None
        K.conv_wgrad(dy.to(dev), x4.to(dev), dw.t, ws.t, R=7, S=7, stride=2, pad=3, stem=True, out_krsc=ok.t if krsc else None)
        if krsc:
            verify(leg, "stem wgrad", dev, ok.t, real[..., :3].contiguous(), None if realb is None else realb[..., :3], what)
            ok.check(what)
        else:
            verify(leg, "stem wgrad", dev, dw.t, full, fullb, what)
        dw.check(what)
        ws.check(what + " workspace")
