"""Parameter groups at the kernel level: ``K.sgd_step`` / ``K.adam_step`` with a run table (``runs=``).

Conventions of tests/test_nn_ops.py (its helpers are imported): every test runs on the CPU (``ops.kernels``
dispatches CPU tensors to ``ops/reference.py``) and on the GPU (the HIP kernels ``sgd_kernel<EMA, true>`` /
``adam_kernel<EMA, true>``); the oracle is the float64 textbook formula written here, with per-element
``wd`` / ``lr_mult`` vectors expanded on the host -- never ``reference.py``, never another kernel; output
buffers start NaN-filled (where the kernel does not read them) inside sentinel guards.

Bounds: exactly test_nn_ops.py's per-element bounds of ``test_sgd_step`` / ``test_adam_step`` (``2^-20`` of
the sum of the absolute values of the chain's terms: 16 fp32 roundings), with ``lr`` replaced by the
exact product ``f32(lr) * f32(lr_mult[r])`` and ``wd`` by ``f32(wd[r])``; the kernel's one extra rounding
of that product is inside the 16-rounding allowance. The fused average: ``e = fma(omd, p - e, e)`` from the
parameter the kernel stored, two roundings, bound ``2^-20 (|e| + omd (|p| + |e|))``.

Where ``lr_mult == 0`` and ``wd == 0`` the parameter is bit-unchanged; a table whose every run is
``(wd0, 1.0)`` gives the bits of the plain kernel called with ``weight_decay=wd0`` (``x * 1.0f`` is exact
and the build has no fast-math), on every output.

The largest err / bound of each test is printed and, with ``$DBX_PARAM_GROUPS_RATIOS`` set, written there
as JSON (profiles/param_groups/test_ratios.json). When this file was introduced (CPU reference path /
MI355X), nothing widened: sgd_groups 0.249 / 0.199, adam_groups 0.128 / 0.131.
"""
import itertools
import json
import os

import pytest
import torch

from dbx_distributed_pytorch_examples_amd.ops import kernels as K
from test_nn_ops import BF, DEVICES, F32, GPU_ONLY, G, f32, f32_bound, gen, rand, randn

devices = pytest.mark.parametrize("dev", DEVICES)
RATIOS = {}
LMS, WDS = (0.0, 0.1, 1.0, 2.5), (0.0, 1e-2)


def report_ratios():
    """Print the largest err / bound per key so far; write them all to ``$DBX_PARAM_GROUPS_RATIOS`` when set
    (tests/test_param_groups_cpu.py and _gpu.py add the trainer-level keys and call this again)."""
    if not RATIOS:
        return
    print("\n[test_param_groups] largest err / bound per test and device:")
    for k in sorted(RATIOS):
        print(f"  {k}: {RATIOS[k]:.4f}")
    path = os.environ.get("DBX_PARAM_GROUPS_RATIOS")
    if path:
        with open(path, "w") as f:
            json.dump(RATIOS, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    report_ratios()


def check(key, dev, got, ref, bound, what=""):
    got = got.detach().double().reshape(ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite (unwritten?) output elements"
    err = (got - ref).abs()
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


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---------------------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------------------
def mixed(starts, shift=0):
    """``[(start, wd, lr_mult)]`` with the values mixed over the runs: every lr_mult of LMS, both decays,
    (0, 0) (parameters held still) and (0, wd) among them once there are 5 runs."""
    return [(s, WDS[((r + shift) // 3) % 2], LMS[(r + shift) % 4]) for r, s in enumerate(starts)]


def ragged(n_total, seed=3):
    """Run lengths of 4..16 elements (multiples of 4) up to ``n_total``."""
    g = torch.Generator().manual_seed(seed)
    starts, s = [], 0
    while s < n_total:
        starts.append(s)
        s += 4 * int(torch.randint(1, 5, (1,), generator=g))
    return starts


def expand(runs, n_total, lo, hi, dev):
    """Per-element float64 (f32(wd), f32(lr_mult)) vectors of [lo, hi), on the host."""
    wd, lm = torch.empty(n_total, dtype=torch.float64), torch.empty(n_total, dtype=torch.float64)
    ends = [r[0] for r in runs[1:]] + [n_total]
    for (s, w, m), e in zip(runs, ends):
        wd[s:e], lm[s:e] = f32(w), f32(m)
    return wd[lo:hi].to(dev), lm[lo:hi].to(dev)


def cases(gpu_n=None):
    """(id, n, runs, n_total, run_base): the sizes and tables at which the grouped kernels can go wrong."""
    out = []
    for n in (4, 5, 20, 1027):
        nt = (n + 3) // 4 * 4
        out.append((f"n{n}-single", n, mixed([0], shift=3), nt, 0))               # one run, (wd, 2.5)
        out.append((f"n{n}-runs4", n, mixed(list(range(0, nt, 4))), nt + 8, 0))    # runs of exactly 4 elements
    # a run boundary at the last full vector, the scalar tail in yet another run
    out.append(("n1027-tail", 1027, mixed([0, 1020, 1024], shift=1), 1027, 0))
    out.append(("n5-tail", 5, mixed([0, 4], shift=2), 5, 0))
    # 300 runs of 4..16 elements: past any 256-entry assumption
    st = ragged(100000)[:300]
    out.append(("runs300", st[-1] + 7, mixed(st), st[-1] + 7, 0))
    # a slice that starts inside one run and ends inside another of a larger buffer's table
    out.append(("base12-n1027", 1027, mixed(list(range(0, 2000, 40))), 2000, 12))
    inside = next(st[i] + 4 for i in range(100, 299) if st[i + 1] - st[i] >= 8)
    out.append(("base300runs-n1027", 1027, mixed(st), st[-1] + 7, inside))
    return [pytest.param(*c[1:], id=c[0]) for c in out]


def state(dev, n, seed):
    g = gen(dev, seed)
    return randn(g, n), randn(g, n), randn(g, n), rand(g, n, lo=0.0, hi=2.0), randn(g, n)


def ema_check(key, dev, e, e0, p, omd, what):
    fo = f32(omd)
    ref = e0.double() + fo * (p.double() - e0.double())
    check(key, dev, e, ref, f32_bound(e0.double().abs() + fo * (p.double().abs() + e0.double().abs())), what + " ema")


# ---------------------------------------------------------------------------------------------
# SGD
# ---------------------------------------------------------------------------------------------
def run_sgd(dev, n, runs, n_total, run_base, combos):
    p0, g_, v0, _, e0 = state(dev, n, 31)
    tab = K.pack_opt_runs(runs, n_total, dev)
    wdv, lmv = expand(runs, n_total, run_base, run_base + n, dev)
    still = (wdv == 0) & (lmv == 0)
    lr, omd = 0.1, 1.0 - 0.99
    flr = f32(lr) * lmv
    gsp = torch.tensor([0.5], device=dev)
    ema_hyper = torch.tensor([omd], device=dev)
    for (nesterov, mom, first), p16_on, hyper_on, gsp_on, ema_on in combos:
        fm, gscale = f32(mom), 0.25
        gs = gscale * (0.5 if gsp_on else 1.0)
        p, v = G(n, F32, dev, init=p0), G(n, F32, dev, init=v0)
        p16 = G(n, BF, dev) if p16_on else None
        e = G(n, F32, dev, init=e0) if ema_on else None
        hyper = torch.tensor([lr], device=dev) if hyper_on else None
        kw = dict(ema=e.t, ema_hyper=ema_hyper if hyper_on else None, ema_one_minus_decay=omd) if ema_on else {}
        K.sgd_step(p.t, g_, v.t, p16.t if p16_on else None, lr=(123.0 if hyper_on else lr), momentum=mom,
                   nesterov=nesterov, first=first, grad_scale_ptr=gsp if gsp_on else None, grad_scale=gscale,
                   hyper=hyper, runs=tab, run_base=run_base, **kw)
        what = (f"n{n} base{run_base} nesterov{int(nesterov)} mom{mom} first{int(first)} p16{int(p16_on)} "
                f"hyper{int(hyper_on)} gsp{int(gsp_on)} ema{int(ema_on)}")
        d = g_.double() * gs + wdv * p0.double()
        dmag = (g_.double() * gs).abs() + (wdv * p0.double()).abs()
        if mom != 0.0:
            if first:
                buf, bmag = d, dmag
            else:
                buf = fm * v0.double() + d
                bmag = (fm * v0.double()).abs() + dmag
            check("sgd_groups", dev, v.t, buf, f32_bound(bmag), what + " buf")
            d, dmag = (d + fm * buf, dmag + fm * bmag) if nesterov else (buf, bmag)
        else:
            assert torch.equal(v.t, v0), what
        check("sgd_groups", dev, p.t, p0.double() - flr * d, f32_bound(p0.double().abs() + flr * dmag), what + " p")
        assert bits_equal(p.t[still], p0[still]), what + ": lr_mult 0 and wd 0 must leave p bit-unchanged"
        p.check(what)
        v.check(what)
        if p16_on:
            assert torch.equal(p16.t, p.t.to(BF)), what
            p16.check(what)
        if ema_on:
            ema_check("sgd_groups", dev, e.t, e0, p.t, omd, what)
            e.check(what)


SGD_MODES = [(False, 0.0, False), (False, 0.9, False), (True, 0.9, False), (False, 0.9, True), (True, 0.9, True)]
SGD_COMBOS = list(itertools.product(SGD_MODES, (True, False), (True, False), (True, False), (True, False)))


@pytest.mark.parametrize("n,runs,n_total,run_base", cases())
@devices
def test_sgd_groups(dev, n, runs, n_total, run_base):
    """One grouped SGD step from a random state: momentum 0 / 0.9, nesterov, first, p16, hyper, gscale_ptr and
    the fused EMA in every combination (80 per case)."""
    run_sgd(dev, n, runs, n_total, run_base, SGD_COMBOS)


@pytest.mark.parametrize("dev", GPU_ONLY)
def test_sgd_groups_grid_stride(dev):
    """Just past a full grid (8192 blocks x 256 lanes x 4 elements): some lanes make a second trip, and the
    scalar tail is resolved there."""
    n = 8192 * 256 * 4 + 5
    starts = list(range(0, n, 699052))  # 13 runs (multiples of 4)
    run_sgd(dev, n, mixed(starts), n, 0, [((True, 0.9, False), True, True, True, True),
                                         ((False, 0.0, False), False, False, False, False)])


# ---------------------------------------------------------------------------------------------
# Adam / AdamW
# ---------------------------------------------------------------------------------------------
def run_adam(dev, n, runs, n_total, run_base, combos):
    p0, g_, m0, v0, e0 = state(dev, n, 32)
    tab = K.pack_opt_runs(runs, n_total, dev)
    wdv, lmv = expand(runs, n_total, run_base, run_base + n, dev)
    still = (wdv == 0) & (lmv == 0)
    lr, b1, b2, eps, omd = 1e-2, 0.9, 0.999, 1e-8, 1.0 - 0.99
    flr, fb1, fb2, feps = f32(lr) * lmv, f32(b1), f32(b2), f32(eps)
    gsp = torch.tensor([0.5], device=dev)
    ema_hyper = torch.tensor([omd], device=dev)
    for decoupled, step, hyper_on, gsp_on, p16_on, ema_on in combos:
        bc1, bc2 = f32(1 - b1 ** step), f32(1 - b2 ** step)
        gscale = 0.25
        gs = gscale * (0.5 if gsp_on else 1.0)
        p, m, v = G(n, F32, dev, init=p0), G(n, F32, dev, init=m0), G(n, F32, dev, init=v0)
        p16 = G(n, BF, dev) if p16_on else None
        e = G(n, F32, dev, init=e0) if ema_on else None
        hyper = torch.tensor([lr, 1 - b1 ** step, 1 - b2 ** step], device=dev) if hyper_on else None
        kw = dict(ema=e.t, ema_hyper=ema_hyper if hyper_on else None, ema_one_minus_decay=omd) if ema_on else {}
        K.adam_step(p.t, g_, m.t, v.t, p16.t if p16_on else None, lr=(123.0 if hyper_on else lr), beta1=b1, beta2=b2,
                    eps=eps, weight_decay=0.0, decoupled=decoupled, step=(999 if hyper_on else step),
                    grad_scale_ptr=gsp if gsp_on else None, grad_scale=gscale, hyper=hyper, runs=tab,
                    run_base=run_base, **kw)
        what = (f"n{n} base{run_base} decoupled{int(decoupled)} step{step} hyper{int(hyper_on)} gsp{int(gsp_on)} "
                f"p16{int(p16_on)} ema{int(ema_on)}")
        gg, gmag = g_.double() * gs, (g_.double() * gs).abs()
        pp, pmag = p0.double(), p0.double().abs()
        if decoupled:
            pp, pmag = pp - flr * wdv * pp, pmag + (flr * wdv * pp).abs()
        else:
            gg, gmag = gg + wdv * pp, gmag + (wdv * pp).abs()
        mm = fb1 * m0.double() + (1 - fb1) * gg
        mmag = (fb1 * m0.double()).abs() + (1 - fb1) * gmag
        vv = fb2 * v0.double() + (1 - fb2) * gg * gg
        vmag = (fb2 * v0.double()).abs() + 2 * (1 - fb2) * gmag * gmag
        den = torch.sqrt(vv / bc2) + feps
        upd = flr * (mm / bc1) / den
        umag = flr * (mmag / bc1) / den + upd.abs() * (1 + 0.5 * vmag / vv.clamp_min(1e-300))
        check("adam_groups", dev, m.t, mm, f32_bound(mmag), what + " m")
        check("adam_groups", dev, v.t, vv, f32_bound(vmag), what + " v")
        check("adam_groups", dev, p.t, pp - upd, f32_bound(pmag + umag), what + " p")
        assert bits_equal(p.t[still], p0[still]), what + ": lr_mult 0 and wd 0 must leave p bit-unchanged"
        for o in (p, m, v):
            o.check(what)
        if p16_on:
            assert torch.equal(p16.t, p.t.to(BF)), what
            p16.check(what)
        if ema_on:
            ema_check("adam_groups", dev, e.t, e0, p.t, omd, what)
            e.check(what)


ADAM_COMBOS = list(itertools.product((True, False), (1, 7), (True, False), (True, False), (True, False), (True, False)))


@pytest.mark.parametrize("n,runs,n_total,run_base", cases())
@devices
def test_adam_groups(dev, n, runs, n_total, run_base):
    """One grouped Adam / AdamW step: decoupled or L2, step 1 / 7, hyper, gscale_ptr, p16 and the fused EMA in
    every combination (64 per case)."""
    run_adam(dev, n, runs, n_total, run_base, ADAM_COMBOS)


@pytest.mark.parametrize("dev", GPU_ONLY)
def test_adam_groups_grid_stride(dev):
    """Just past a full grid (8192 blocks x 256 lanes, one element each): some lanes make a second trip."""
    n = 8192 * 256 + 5
    starts = list(range(0, n, 174764))  # 13 runs (multiples of 4)
    run_adam(dev, n, mixed(starts), n, 0, [(True, 7, True, True, True, True), (False, 1, False, False, False, False)])


# ---------------------------------------------------------------------------------------------
# bit identity with the plain kernels
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev,n", [("cpu", 5), ("cpu", 1027)] + [pytest.param("cuda", n, marks=pytest.mark.gpu)
                                                                   for n in (5, 1027, 8192 * 256 * 4 + 5)])
def test_trivial_table_is_the_plain_kernel(dev, n):
    """Every run ``(wd0, 1.0)`` against the plain call with ``weight_decay=wd0``: p, state, p16 and ema are
    bit-identical, for SGD, Adam (L2) and AdamW (decoupled), with a table of several runs and a base."""
    wd0, base = 1e-2, 8
    nt = base + n + 3
    tab = K.pack_opt_runs([(s, wd0, 1.0) for s in range(0, nt, max(4, nt // 7 // 4 * 4))], nt, dev)
    p0, g_, m0, v0, e0 = state(dev, n, 33)
    gsp = torch.tensor([0.5], device=dev)

    def outs(fn, **kw):
        bufs = [G(n, F32, dev, init=x) for x in (p0, m0, v0, e0)] + [G(n, BF, dev)]
        p, m, v, e, p16 = bufs
        fn(p, m, v, p16, dict(ema=e.t, ema_one_minus_decay=0.01, grad_scale_ptr=gsp, grad_scale=0.25, **kw))
        for b in bufs:
            b.check(str(kw))
        return [b.t for b in bufs]

    variants = {
        "sgd": lambda nes: (lambda p, m, v, p16, kw: K.sgd_step(p.t, g_, m.t, p16.t, lr=0.1, momentum=0.9,
                                                                  nesterov=nes, **kw)),
        "adam": lambda dec: (lambda p, m, v, p16, kw: K.adam_step(p.t, g_, m.t, v.t, p16.t, lr=1e-2, beta1=0.9,
                                                                   beta2=0.999, eps=1e-8, decoupled=dec, step=3, **kw)),
    }
    for name, flag in (("sgd", False), ("sgd", True), ("adam", False), ("adam", True)):
        fn = variants[name](flag)
        plain = outs(fn, weight_decay=wd0)
        grouped = outs(fn, weight_decay=0.0, runs=tab, run_base=base)
        for a, b, nm in zip(plain, grouped, ("p", "m", "v", "ema", "p16")):
            if name == "sgd" and nm == "v":  # (SGD has one state buffer: "m" above)
                continue
            same = torch.equal(a.view(torch.int16), b.view(torch.int16)) if a.dtype == BF else bits_equal(a, b)
            assert same, f"{name} flag{int(flag)} n{n}: {nm} differs from the plain kernel's"


# ---------------------------------------------------------------------------------------------
# wrapper errors
# ---------------------------------------------------------------------------------------------
@devices
def test_wrapper_errors(dev):
    n = 64
    p, g_, m, v, _ = state(dev, n, 34)
    tab = K.pack_opt_runs([(0, 0.0, 1.0), (32, 1e-2, 0.5)], 96, dev)

    def sgd(**kw):
        a = dict(lr=0.1, momentum=0.9, runs=tab, run_base=0)
        a.update(kw)
        K.sgd_step(p.clone(), g_, m.clone(), **a)

    def adam(**kw):
        a = dict(lr=0.1, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, decoupled=True, step=1, runs=tab, run_base=0)
        a.update(kw)
        K.adam_step(p.clone(), g_, m.clone(), v.clone(), **a)

    for call in (sgd, adam):
        call()                    # the valid call
        call(run_base=32)         # [32, 96): ends exactly at n_total
        with pytest.raises(ValueError, match="multiple of 4"):
            call(run_base=2)
        with pytest.raises(ValueError, match="covers"):
            call(run_base=36)     # 36 + 64 > 96: the table does not cover the slice
        with pytest.raises(ValueError, match="covers"):
            call(run_base=-4)
        with pytest.raises(ValueError, match="weight_decay"):
            call(weight_decay=1e-2)
        with pytest.raises(TypeError):
            call(runs=[(0, 0.0, 1.0)])
        # hand-built tables are validated too (once per tensor object)
        bad = tab.clone()
        bad[1] = 30               # a start that is no multiple of 4
        with pytest.raises(ValueError, match="multiple of 4"):
            call(runs=bad)
        bad = tab.clone()
        bad[0], bad[1] = 32, 0    # unsorted
        with pytest.raises(ValueError):
            call(runs=bad)
    with pytest.raises(ValueError, match="multiple of 4"):
        K.pack_opt_runs([(0, 0.0, 1.0), (6, 0.0, 1.0)], 96, dev)
    with pytest.raises(ValueError, match="increasing"):
        K.pack_opt_runs([(0, 0.0, 1.0), (32, 0.0, 1.0), (16, 0.0, 1.0)], 96, dev)
    with pytest.raises(ValueError, match="increasing"):
        K.pack_opt_runs([(0, 0.0, 1.0), (96, 0.0, 1.0)], 96, dev)  # an empty last run
    with pytest.raises(ValueError, match="start at 0"):
        K.pack_opt_runs([(4, 0.0, 1.0)], 96, dev)
    with pytest.raises(ValueError, match="finite"):
        K.pack_opt_runs([(0, float("nan"), 1.0)], 96, dev)
    with pytest.raises(ValueError, match="finite"):
        K.pack_opt_runs([(0, 0.0, -1.0)], 96, dev)
    assert K.OPT_MAX_RUNS >= 1024
    K.pack_opt_runs([(4 * r, 0.0, 1.0) for r in range(K.OPT_MAX_RUNS)], 4 * K.OPT_MAX_RUNS, dev)
    with pytest.raises(ValueError, match="at most"):
        K.pack_opt_runs([(4 * r, 0.0, 1.0) for r in range(K.OPT_MAX_RUNS + 1)], 4 * K.OPT_MAX_RUNS + 4, dev)


@devices
def test_table_is_validated_once(dev, monkeypatch):
    """A packed table is never read back by a step: the verdict rides on the tensor object."""
    tab = K.pack_opt_runs([(0, 0.0, 1.0), (32, 1e-2, 0.5)], 64, dev)
    p, g_, m, _, _ = state(dev, 64, 35)
    monkeypatch.setattr(torch.Tensor, "tolist", lambda self: (_ for _ in ()).throw(AssertionError("table read back")))
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (_ for _ in ()).throw(AssertionError("table read back")))
    for _ in range(2):
        K.sgd_step(p, g_, m, lr=0.1, momentum=0.9, runs=tab, run_base=0)


@pytest.mark.parametrize("dev", GPU_ONLY)
def test_max_runs_table(dev):
    """The largest table the kernels take (1024 runs of 4 elements, all of LDS's arrays in use)."""
    n = 4 * K.OPT_MAX_RUNS + 3
    run_sgd(dev, n, mixed(list(range(0, 4 * K.OPT_MAX_RUNS, 4))), n, 0, [((True, 0.9, False), True, True, True, True)])
    run_adam(dev, n, mixed(list(range(0, 4 * K.OPT_MAX_RUNS, 4))), n, 0, [(True, 7, True, True, True, True)])
