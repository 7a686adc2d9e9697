"""``ce_eval`` (loss and label-rank metrics without a gradient) and ``bn_eval_coeff_multi`` (every
BatchNorm's eval coefficients in one launch), per element, on the CPU reference and on the HIP kernels.

The oracle is float64 torch of the definitions, written here: for a row with label l,
``rank = #{c : x_c > x_l} + #{c < l : x_c == x_l}`` and ``loss = lse(x) - x_l``. Ranks and the three
counters are exact. Bounds of the loss, derived as in tests/test_nn_ops.py:

* per row, the plain fp32 bound of an elementwise chain, ``2^-20 (|lse| + |x_l|)`` (what that file's
  header says ``softmax_ce``'s loss keeps; nothing is widened for the exponential);
* the loss sum: the rows' bounds added up, plus ``sum_bound(n, sum |loss|)`` for a sum of n fp32 terms
  in any order (the reference adds in fp64, the kernel adds fp32 losses with fp64 atomics: both inside),
  plus ``(n + 2) 2^-53`` of the fp64 accumulator's magnitude.

Outputs start as NaN / a sentinel inside guard elements that must be unchanged afterwards. Every check
prints its largest err / bound (``-s`` shows them; the module's maxima are printed at its end).
"""
import math

import pytest
import torch

from dbx_distributed_pytorch_examples_amd.ops import kernels as K

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
devices = pytest.mark.parametrize("dev", DEVICES)
BF, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32
U_CHAIN = 2.0 ** -20   # 16 fp32 roundings (tests/test_nn_ops.py)
BS = [1, 3, 130]
CS = [1, 10, 63, 64, 65, 255, 256, 257, 1000, 1001]
DTYPES = pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
STATS0 = [3.5, 2.0, 7.0, 11.0]  # the counters add to what is there
RATIOS = {}

_INT = {F32: torch.int32, F64: torch.int64, I32: torch.int32}
_SENTINEL = {F32: 0x7FC0A5A5, F64: 0x7FF8A5A5A5A5A5A5, I32: 0x5A5A5A5A}
GUARD = 64


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    if RATIOS:
        print("\n[test_ce_eval] largest err / bound per check and device:")
        for k in sorted(RATIOS):
            print(f"  {k}: {RATIOS[k]:.4f}")


def sum_bound(n, sum_abs):
    return (n * 2.0 ** -24 + 2.0 ** -21) * sum_abs


class Guarded:
    """``t`` of ``n`` elements inside a larger allocation whose guard elements hold a sentinel; ``t`` starts
    as NaN (floats), as the sentinel itself (int32), or as ``init``."""

    def __init__(self, n, dtype, dev, init=None):
        self.n, self.dtype = n, dtype
        self.buf = torch.empty(n + 2 * GUARD, dtype=dtype, device=dev)
        self.bits = self.buf.view(_INT[dtype])
        self.bits.fill_(_SENTINEL[dtype])
        self.t = self.buf[GUARD:GUARD + n]
        if init is not None:
            self.t.copy_(torch.as_tensor(init, dtype=dtype))
        elif dtype != I32:
            self.t.fill_(float("nan"))

    def check(self, what=""):
        g = torch.cat([self.bits[:GUARD], self.bits[GUARD + self.n:]])
        assert bool((g == _SENTINEL[self.dtype]).all()), f"{what}: wrote outside the output region"


def check(key, dev, got, ref, bound, what=""):
    got = got.detach().double().reshape(ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite (unwritten?) output elements"
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"{key}[{dev}] {what}: max err/bound = {worst:.4f}")
    RATIOS[f"{key}[{dev}]"] = max(RATIOS.get(f"{key}[{dev}]", 0.0), worst)
    assert worst <= 1.0, f"{what}: err / bound = {worst:.3f} at element {int(ratio.flatten().argmax())}"


def gen(dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return g


def oracle(x, labels, k, nvalid):
    """float64: (valid, rank, loss, per-row loss bound). Rows that are not valid hold rank -1, loss 0."""
    B, C = x.shape
    dev = x.device
    x64 = x.double()
    valid = (labels >= 0) & (labels < C) & (torch.arange(B, device=dev) < nvalid)
    lab = torch.where(valid, labels, torch.zeros_like(labels))[:, None]
    xl = x64.gather(1, lab)
    idx = torch.arange(C, device=dev)[None, :]
    rank = ((x64 > xl) | ((x64 == xl) & (idx < lab))).sum(1)
    mx = x64.max(1, keepdim=True).values
    lse = (mx + torch.log(torch.exp(x64 - mx).sum(1, keepdim=True))).squeeze(1)
    xl = xl.squeeze(1)
    loss = lse - xl
    bound = U_CHAIN * (lse.abs() + xl.abs())
    zero = torch.zeros_like(loss)
    return (valid, torch.where(valid, rank, torch.full_like(rank, -1)), torch.where(valid, loss, zero),
            torch.where(valid, bound, zero))


def run_and_check(dev, x, labels, k, nvalid, what):
    """One ce_eval call with every output, against the oracle."""
    B, C = x.shape
    valid, rank, loss, lbound = oracle(x, labels, k, B if nvalid is None else nvalid)
    st = Guarded(4, F64, dev, init=STATS0)
    lo = Guarded(B, F32, dev)
    ro = Guarded(B, I32, dev)
    nv = None if nvalid is None else torch.tensor([nvalid], dtype=I32, device=dev)
    K.ce_eval(x, labels, st.t, k, nvalid=nv, loss_out=lo.t, rank_out=ro.t)
    for g in (st, lo, ro):
        g.check(what)
    assert torch.equal(ro.t.long(), rank), f"{what}: rank_out"
    n = int(valid.sum())
    want = [float((valid & (rank < 1)).sum()), float((valid & (rank < k)).sum()), float(n)]
    assert st.t[1:].tolist() == [a + b for a, b in zip(STATS0[1:], want)], f"{what}: counters"
    assert bool((lo.t[~valid] == 0).all()), f"{what}: an ignored row's loss_out is not 0"
    check("ce_eval loss", dev, lo.t, loss, lbound, what)
    sabs = float(loss.abs().sum())
    sbound = float(lbound.sum()) + sum_bound(n, sabs) + (n + 2) * 2.0 ** -53 * (STATS0[0] + sabs)
    check("ce_eval loss sum", dev, st.t[0:1] - STATS0[0], loss.sum().reshape(1), torch.tensor([sbound], dtype=F64, device=dev),
          what)
    # the optional outputs left out: the same sums
    st2 = Guarded(4, F64, dev, init=STATS0)
    K.ce_eval(x, labels, st2.t, k, nvalid=nv)
    st2.check(what)
    assert st2.t[1:].tolist() == st.t[1:].tolist(), f"{what}: counters without the per-row outputs"
    check("ce_eval loss sum", dev, st2.t[0:1] - STATS0[0], loss.sum().reshape(1),
          torch.tensor([sbound], dtype=F64, device=dev), what + " (no per-row outputs)")


def ks(C):
    return sorted({1, min(5, C), C})


def tie_rows(g, B, C, dev, shift):
    """Logits from five small integers (most rows hold ties) and, per row, a label at the first, a middle
    or the last position of its tie group (row r: position kind (r + shift) % 3)."""
    x = torch.randint(-2, 3, (B, C), generator=g, device=dev).float()
    pick = torch.randint(0, C, (B,), generator=g, device=dev)
    labels = torch.empty(B, dtype=torch.int64, device=dev)
    for r in range(B):
        grp = (x[r] == x[r, pick[r]]).nonzero().flatten()
        labels[r] = grp[(0, len(grp) // 2, len(grp) - 1)[(r + shift) % 3]]
    return x, labels


@DTYPES
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("B", BS)
@devices
def test_ce_eval_random(dev, B, C, dtype):
    g = gen(dev, 100 * B + C)
    x = (torch.randn(B, C, generator=g, device=dev) * 2.0).to(dtype)
    labels = torch.randint(0, C, (B,), generator=g, device=dev)
    for k in ks(C):
        run_and_check(dev, x, labels, k, None, f"random B{B} C{C} k{k}")


@DTYPES
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("B", BS)
@devices
def test_ce_eval_ties(dev, B, C, dtype):
    g = gen(dev, 7 * B + C)
    for shift in range(3):  # every row meets every position of its tie group
        x, labels = tie_rows(g, B, C, dev, shift)
        for k in ks(C):
            run_and_check(dev, x.to(dtype), labels, k, None, f"ties B{B} C{C} k{k} shift{shift}")
    # a row whose elements are all equal: rank = label
    x = torch.full((B, C), 1.25, device=dev).to(dtype)
    for lab in sorted({0, C // 2, C - 1}):
        labels = torch.full((B,), lab, dtype=torch.int64, device=dev)
        for k in ks(C):
            run_and_check(dev, x, labels, k, None, f"all equal B{B} C{C} k{k} label{lab}")


@DTYPES
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("B", BS)
@devices
def test_ce_eval_masking(dev, B, C, dtype):
    g = gen(dev, 13 * B + C)
    x = (torch.randn(B, C, generator=g, device=dev) * 2.0).to(dtype)
    good = torch.randint(0, C, (B,), generator=g, device=dev)
    bad = good.clone()
    outside = [-1, C, 2 ** 40 + 3]
    for i, r in enumerate(range(0, B, 3)):  # labels outside [0, C) are never used as an index
        bad[r] = outside[i % 3]
    k = min(5, C)
    for nvalid in sorted({0, 1, B - 1, B}):
        run_and_check(dev, x, good, k, nvalid, f"nvalid {nvalid} B{B} C{C}")
        run_and_check(dev, x, bad, k, nvalid, f"nvalid {nvalid}, bad labels B{B} C{C}")
    run_and_check(dev, x, bad, k, None, f"bad labels B{B} C{C}")
    # nothing counted: the statistics are untouched, bit for bit
    st = Guarded(4, F64, dev, init=STATS0)
    K.ce_eval(x, good, st.t, k, nvalid=torch.zeros(1, dtype=I32, device=dev))
    assert st.t.tolist() == STATS0
    st.check()


@DTYPES
@pytest.mark.parametrize("C", [1, 10, 257, 1000])
@devices
def test_ce_eval_nan_label_logit(dev, C, dtype):
    """A NaN label logit: a miss at every k (rank_out = C) and a NaN loss; the other rows are unaffected."""
    g = gen(dev, C)
    B = 5
    x = (torch.randn(B, C, generator=g, device=dev) * 2.0).to(dtype)
    labels = torch.randint(0, C, (B,), generator=g, device=dev)
    x[2, labels[2]] = float("nan")
    _, rank, _, _ = oracle(x, labels, C, B)
    st = Guarded(4, F64, dev, init=[0.0, 0.0, 0.0, 0.0])
    lo, ro = Guarded(B, F32, dev), Guarded(B, I32, dev)
    K.ce_eval(x, labels, st.t, C, loss_out=lo.t, rank_out=ro.t)
    for gd in (st, lo, ro):
        gd.check()
    keep = torch.arange(B, device=dev) != 2
    assert int(ro.t[2]) == C and math.isnan(float(lo.t[2]))
    assert torch.equal(ro.t[keep].long(), rank[keep]) and bool(torch.isfinite(lo.t[keep]).all())
    s = st.t.tolist()
    assert math.isnan(s[0]) and s[3] == B
    assert s[1] == float((rank[keep] < 1).sum()) and s[2] == B - 1  # k = C: every other row is a hit


@devices
def test_ce_eval_bad_arguments(dev):
    x = torch.zeros(3, 10, device=dev)
    lab = torch.zeros(3, dtype=torch.int64, device=dev)
    st = torch.zeros(4, dtype=F64, device=dev)
    for k in (0, 11, -1):
        with pytest.raises(ValueError):
            K.ce_eval(x, lab, st, k)
    with pytest.raises(TypeError):
        K.ce_eval(x.half(), lab, st, 1)
    with pytest.raises(TypeError):
        K.ce_eval(x, lab.int(), st, 1)
    with pytest.raises(TypeError):
        K.ce_eval(x, lab, st.float(), 1)
    with pytest.raises(ValueError):
        K.ce_eval(x, lab, torch.zeros(2, dtype=F64, device=dev), 1)
    with pytest.raises(ValueError):
        K.ce_eval(x, lab[:2], st, 1)
    with pytest.raises(TypeError):
        K.ce_eval(x, lab, st, 1, nvalid=torch.zeros(1, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError):
        K.ce_eval(x, lab, st, 1, rank_out=torch.zeros(2, dtype=I32, device=dev))
    assert st.tolist() == [0.0] * 4


@DTYPES
@pytest.mark.parametrize("C", [10, 257, 1000])
@devices
def test_ce_eval_top1_is_softmax_ce_correct(dev, C, dtype):
    """stats[1] counts exactly what the training kernel's ``correct`` counts, ties included."""
    g = gen(dev, 5 * C)
    B = 130
    xr = (torch.randn(B, C, generator=g, device=dev) * 2.0).to(dtype)
    lr = xr.float().argmax(1)
    lr[::2] = torch.randint(0, C, (B,), generator=g, device=dev)[::2]  # about half of the rows correct
    xt, lt = tie_rows(g, B, C, dev, 0)
    for x, labels in ((xr, lr), (xt.to(dtype), lt)):
        tr = torch.zeros(2, dtype=F64, device=dev)
        K.softmax_ce(x, labels, None, None, tr)
        ev = torch.zeros(4, dtype=F64, device=dev)
        K.ce_eval(x, labels, ev, 1)
        assert float(ev[1]) == float(tr[1]) and float(ev[2]) == float(tr[1]) and float(ev[3]) == B
        assert 0 < float(ev[1]) < B


# ---------------------------------------------------------------------------------------------
# bn_eval_coeff_multi
# ---------------------------------------------------------------------------------------------
@devices
def test_bn_eval_coeff_multi(dev):
    """Mixed widths and every gamma / beta combination in one table: the bits of one bn_eval_coeff per BN."""
    g = gen(dev, 3)
    widths = [64, 128, 512, 2048, 64, 3, 300, 2048]
    entries, want, outs = [], [], []
    for i, C in enumerate(widths):
        gamma = torch.randn(C, generator=g, device=dev) if i % 2 == 0 else None
        beta = torch.randn(C, generator=g, device=dev) if i % 4 < 2 else None
        rm = torch.randn(C, generator=g, device=dev)
        rv = torch.rand(C, generator=g, device=dev) + 0.05
        eps = (1e-5, 1e-3)[i % 2]
        sc, sh = Guarded(C, F32, dev), Guarded(C, F32, dev)
        entries.append((gamma, beta, eps, rm, rv, sc.t, sh.t))
        outs.append((sc, sh))
        s1, s2 = torch.empty(C, device=dev), torch.empty(C, device=dev)
        K.bn_eval_coeff(gamma, beta, eps, rm, rv, s1, s2)
        want.append((s1, s2))
        # (and the single kernel against float64: it is the reference of the table-driven one)
        inv = 1.0 / torch.sqrt(rv.double() + float(torch.tensor(eps, dtype=F32)))
        g64 = gamma.double() if gamma is not None else torch.ones(C, dtype=F64, device=dev)
        b64 = beta.double() if beta is not None else torch.zeros(C, dtype=F64, device=dev)
        check("bn_eval_coeff", dev, s1, g64 * inv, U_CHAIN * (g64 * inv).abs(), f"scale C{C}")
        check("bn_eval_coeff", dev, s2, b64 - rm.double() * g64 * inv,
              U_CHAIN * (b64.abs() + (rm.double() * g64 * inv).abs()), f"shift C{C}")
    table, n, mx = K.pack_bn_eval_desc(entries, dev)
    assert (n, mx) == (len(widths), 2048) and table.numel() == 56 * n
    K.bn_eval_coeff_multi(table, n, mx)
    for (sc, sh), (s1, s2), C in zip(outs, want, widths):
        assert torch.equal(sc.t, s1) and torch.equal(sh.t, s2), f"width {C}"
        sc.check(f"scale C{C}")
        sh.check(f"shift C{C}")
    with pytest.raises(TypeError):
        K.pack_bn_eval_desc([(None, None, 1e-5, entries[0][3].double(), entries[0][4], outs[0][0].t, outs[0][1].t)], dev)
    with pytest.raises(ValueError):
        K.pack_bn_eval_desc([(None, None, 1e-5, entries[1][3], entries[0][4], outs[0][0].t, outs[0][1].t)], dev)
    with pytest.raises(ValueError):
        K.bn_eval_coeff_multi(table, n + 1, mx)


@devices
def test_program_bn_tables(dev):
    """The program's table covers every BN and reproduces the per-BN launches of an eval forward."""
    from dbx_distributed_pytorch_examples_amd.engine.program import ResNetProgram
    from dbx_distributed_pytorch_examples_amd.models import resnet18
    torch.manual_seed(0)
    model = resnet18(num_classes=10).to(dev)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_()
            m.running_var.uniform_(0.5, 2.0)
    p = ResNetProgram(model, 2, (32, 32), torch.device(dev))
    assert p.bn_eval_table[1] == len(p.bns) == 20
    want = []
    for bn in p.bns:
        K.bn_eval_coeff(bn.gamma, bn.beta, bn.mod.eps, bn.mod.running_mean, bn.mod.running_var, bn.scale, bn.shift)
        want.append((bn.scale.clone(), bn.shift.clone()))
    p.bn_arena.fill_(float("nan"))
    p.bn_eval_coeffs()
    for bn, (sc, sh) in zip(p.bns, want):
        assert torch.equal(bn.scale, sc) and torch.equal(bn.shift, sh), bn.name
