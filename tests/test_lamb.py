"""LAMB in the native training step: the ``lamb_step`` kernels per element, the fused EMA variant, the
torch ``LAMB`` class, the trainer plumbing and the configuration layers.

Conventions of tests/test_nn_ops.py (its helpers are imported): every kernel test runs on the CPU
(``ops.kernels`` dispatches CPU tensors to ``ops/reference.py``) and on the GPU (the HIP kernels); the
oracle is float64 torch of the formula, written here (``seg_oracle``), never ``reference.py``; output
buffers sit inside sentinel guards; bounds are derived per element and the largest err / bound of each
test is printed (and written as JSON to ``$DBX_LAMB_RATIOS`` when set).

The formula, per tensor (w the master, g the gradient, gs the gradient scale):

    gg = gs*g;  m = b1*m + (1-b1)*gg;  v = b2*v + (1-b2)*gg*gg
    r  = (m/bc1) / (sqrt(v/bc2) + eps)
    u  = adapt ? r + wd*w : r
    t  = adapt && |w|>0 && |u|>0 ? |w|/|u| : 1;  t = clamp(t, trust_min, trust_max) where adapted
    w -= lr*t*u

Bounds (``U = 2^-20``, the 16 fp32 roundings of test_nn_ops):

* m, v, r exactly as test_adam_step derives them; u adds ``|wd*w|`` to r's magnitude: ``|u - u*| <= U umag``;
* a squared norm of n fp32 terms: relative ``s(n) = n 2^-24 + 2^-21`` (any summation order; the fp64
  sum over the blocks' partials adds nothing visible); |u|^2 is formed from the kernel's own u, so the
  elements' bounds enter squared on top: ``sum(2 |u| bu + bu^2) / |u|^2``;
* t = sqrt(|w|^2 / |u|^2): relative ``rel(t) = s(n)/2 + (s(n) + sum(2 |u| bu + bu^2) / |u|^2)/2 + U`` (the
  square roots, their fp32 casts and the division); 0 where t is the constant 1 or a clamp value;
* p: ``U (|w| + |lr t u|) + |lr t u| rel(t) + lr t bu``.

Largest err / bound seen when this file was introduced (CPU reference path / MI355X), nothing widened:
kernel sweep m 0.121 / 0.097, v 0.123 / 0.062, u 0.138 / 0.114, p 0.107 / 0.092; trainer m 0.121 / 0.161,
v 0.123 / 0.143, p 0.069 / 0.064, clip factor 0.032 / 0.030.
"""
import copy
import itertools
import json
import os
from types import SimpleNamespace

import pytest
import torch

from dbx_distributed_pytorch_examples_amd.engine.autograd_trainer import LAMB, build_torch_optimizer
from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig
from dbx_distributed_pytorch_examples_amd.models import build_model
from dbx_distributed_pytorch_examples_amd.ops import kernels as K
from dbx_distributed_pytorch_examples_amd.ops import reference as R
from test_nn_ops import BF, DEVICES, F32, F64, GPU_ONLY, U_CHAIN, G, f32, f32_bound, gen, rand, randn

devices = pytest.mark.parametrize("dev", DEVICES)
RATIOS = {}
B1, B2 = 0.9, 0.999


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    if not RATIOS:
        return
    print("\n[test_lamb] largest err / bound per test and device:")
    for k in sorted(RATIOS):
        print(f"  {k}: {RATIOS[k]:.4f}")
    path = os.environ.get("DBX_LAMB_RATIOS")
    if path:
        with open(path, "w") as f:
            json.dump(RATIOS, f, indent=1, sort_keys=True)


def check(key, dev, got, ref, bound, what=""):
    """test_nn_ops.check with this module's RATIOS (and no print per call: the sweeps are long)."""
    got = got.detach().double().reshape(ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite (unwritten?) output elements"
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    k = f"{key}[{dev}]"
    RATIOS[k] = max(RATIOS.get(k, 0.0), worst)
    if not worst <= 1.0:
        i = int(ratio.flatten().argmax())
        raise AssertionError(f"{what}: element {i}: got {got.flatten()[i].item()!r}, want {ref.flatten()[i].item()!r}, "
                             f"err {err.flatten()[i].item():.3e} > bound {bound.flatten()[i].item():.3e} "
                             f"(ratio {worst:.3f}; {int((ratio > 1).sum())} of {ratio.numel()} elements out)")


# ---------------------------------------------------------------------------------------------
# the float64 oracle of one tensor, with its bounds
# ---------------------------------------------------------------------------------------------
def s_rel(n):
    return n * 2.0 ** -24 + 2.0 ** -21


def seg_oracle(w, g, m0, v0, adapt, o):
    """``o``: lr, b1, b2, eps, wd, bc1, bc2, gs, tmin, tmax as the fp32 values the kernel sees (Python
    floats). Returns the new m, v, the u left in g, the raw and the applied trust ratio, the new p, and
    the bounds of m, v, u, p."""
    w, g, m0, v0 = w.double(), g.double(), m0.double(), v0.double()
    gg, gmag = g * o.gs, (g * o.gs).abs()
    mm = o.b1 * m0 + (1 - o.b1) * gg
    mmag = (o.b1 * m0).abs() + (1 - o.b1) * gmag
    vv = o.b2 * v0 + (1 - o.b2) * gg * gg
    vmag = (o.b2 * v0).abs() + 2 * (1 - o.b2) * gmag * gmag  # (gg's own error enters squared)
    den = torch.sqrt(vv / o.bc2) + o.eps
    r = (mm / o.bc1) / den
    # the numerator's terms over the denominator, plus the denominator's own relative error (half of
    # vv's through the square root) on the quotient
    rmag = (mmag / o.bc1) / den + r.abs() * (1 + 0.5 * vmag / vv.clamp_min(1e-300))
    u, umag = (r + o.wd * w, rmag + (o.wd * w).abs()) if adapt else (r, rmag)
    ub = f32_bound(umag)
    raw = t = 1.0
    rel_t = 0.0
    if adapt:
        n = w.numel()
        W2, U2 = float((w * w).sum()), float((u * u).sum())
        if W2 > 0 and U2 > 0:
            raw = t = (W2 / U2) ** 0.5
            rel_t = 0.5 * s_rel(n) + 0.5 * (s_rel(n) + float((2 * u.abs() * ub + ub * ub).sum()) / U2) + U_CHAIN
        if o.tmin > 0 and t < o.tmin:
            t, rel_t = o.tmin, 0.0
        if o.tmax > 0 and t > o.tmax:
            t, rel_t = o.tmax, 0.0
    step = o.lr * t * u
    p = w - step
    pb = f32_bound(w.abs() + step.abs()) + step.abs() * rel_t + o.lr * t * ub
    return SimpleNamespace(m=mm, mb=f32_bound(mmag), v=vv, vb=f32_bound(vmag), u=u, ub=ub, raw=raw, t=t, p=p, pb=pb)


def table(lens, adapt, dev):
    """Segments at 16-element aligned offsets (the program's layout): int32 device tables + total size."""
    offs, o = [], 0
    for n in lens:
        offs.append(o)
        o += (n + 15) // 16 * 16
    it = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)  # noqa: E731
    return offs, it(offs), it(lens), it(adapt), max(o, 16)


def seg_index(offs, lens, total, dev):
    idx = torch.cat([torch.arange(o, o + n, device=dev) for o, n in zip(offs, lens)])
    gap = torch.ones(total, dtype=torch.bool, device=dev)
    gap[idx] = False
    return idx, gap


def norms_buf(nseg, dev):
    return torch.zeros(K.LARS_MAX_BLOCKS * 2 * nseg, dtype=F64, device=dev)


# ---------------------------------------------------------------------------------------------
# 1. the kernels, per element
# ---------------------------------------------------------------------------------------------
# scalar tail only (1, 3), one vector (4), vector + tail (5, 10, 1027), one block (64, 1000), several
# blocks (4096), the block cap and a grid-stride loop that runs more than once (65548 = 64 blocks x 256
# lanes x 4 + 12; 300000); then an adapted tensor of all-zero w and one with g = m = 0
LENS = [1, 3, 4, 5, 10, 64, 1000, 1027, 4096, 65548, 300000, 100, 37]
ADAPT = [1, 0, 1, 1, 0, 1, 0, 1, 1, 0, 1, 1, 1]
ZERO_W, ZERO_U = 11, 12
GAP = 12345.0  # what the alignment gaps between the tensors hold (must stay)
TMIN_SAT, TMAX_SAT = 1e4, 1e-4  # saturating clamps: every unclamped ratio below is inside (1e-2, 1e2)


def _state(dev, seed=21):
    offs, off, ln, ad, total = table(LENS, ADAPT, dev)
    idx, gap = seg_index(offs, LENS, total, dev)
    g = gen(dev, seed)
    w, gr, m, v = randn(g, total), randn(g, total), randn(g, total), rand(g, total, lo=0.01, hi=2.0)
    o, n = offs[ZERO_W], LENS[ZERO_W]
    w[o:o + n] = 0.0
    o, n = offs[ZERO_U], LENS[ZERO_U]
    gr[o:o + n] = 0.0
    m[o:o + n] = 0.0
    for t in (w, gr, m, v):
        t[gap] = GAP
    return offs, off, ln, ad, total, idx, gap, w, gr, m, v


@pytest.mark.parametrize("clamp", ["off", "low", "high"])
@devices
def test_lamb_step(dev, clamp):
    """One step from a random state over the 13-tensor table, every option combination (32 per clamp
    mode): m, v, the u left in g, p and the bf16 copy against the float64 oracle."""
    offs, off, ln, ad, total, idx, gap, w0, g0, m0, v0 = _state(dev)
    lr, eps = 1e-2, 1e-8
    tmin, tmax = {"off": (0.0, 0.0), "low": (TMIN_SAT, 0.0), "high": (0.0, TMAX_SAT)}[clamp]
    gsp = torch.tensor([0.5], device=dev)
    for wd, step, hyper_on, gsp_on, p16_on in itertools.product((0.0, 1e-2), (1, 7), (True, False), (True, False),
                                                                (True, False)):
        gscale = 0.25
        o = SimpleNamespace(lr=f32(lr), b1=f32(B1), b2=f32(B2), eps=f32(eps), wd=f32(wd), bc1=f32(1 - B1 ** step),
                            bc2=f32(1 - B2 ** step), gs=gscale * (0.5 if gsp_on else 1.0), tmin=f32(tmin), tmax=f32(tmax))
        p, g, m, v = (G(total, F32, dev, init=x) for x in (w0, g0, m0, v0))
        p16 = G(total, BF, dev) if p16_on else None
        norms = norms_buf(len(LENS), dev)
        hyper = torch.tensor([lr, 1 - B1 ** step, 1 - B2 ** step], device=dev) if hyper_on else None
        K.lamb_step(p.t, g.t, m.t, v.t, off, ln, ad, norms, p16.t if p16_on else None, lr=(123.0 if hyper_on else lr),
                    beta1=B1, beta2=B2, eps=eps, weight_decay=wd, step=(999 if hyper_on else step), trust_min=tmin,
                    trust_max=tmax, grad_scale_ptr=gsp if gsp_on else None, grad_scale=gscale, hyper=hyper,
                    max_len=max(LENS))
        what = f"clamp-{clamp} wd{wd} step{step} hyper{int(hyper_on)} gsp{int(gsp_on)} p16{int(p16_on)}"
        for s, (a, n, adapt) in enumerate(zip(offs, LENS, ADAPT)):
            sl = slice(a, a + n)
            r = seg_oracle(w0[sl], g0[sl], m0[sl], v0[sl], adapt, o)
            if adapt and s not in (ZERO_W, ZERO_U):  # the oracle and the kernel cannot fall on different sides
                assert 100 * TMAX_SAT < r.raw < TMIN_SAT / 100, (what, s, r.raw)
            if s == ZERO_W or (s == ZERO_U and wd == 0.0):
                assert r.raw == 1.0, (what, s)
                if clamp == "off":  # t = 1: the parameter moves by exactly lr * u
                    assert r.t == 1.0
            if s == ZERO_U and wd == 0.0:
                assert float(g.t[sl].abs().max()) == 0.0 and torch.equal(p.t[sl], w0[sl]), what
            tag = f"{what} tensor{s}(n={n})"
            check("lamb_step m", dev, m.t[sl], r.m, r.mb, tag + " m")
            check("lamb_step v", dev, v.t[sl], r.v, r.vb, tag + " v")
            check("lamb_step u", dev, g.t[sl], r.u, r.ub, tag + " u")
            check("lamb_step p", dev, p.t[sl], r.p, r.pb, tag + " p")
        for buf, init in ((p, w0), (g, g0), (m, m0), (v, v0)):
            buf.check(what)
            assert torch.equal(buf.t[gap], init[gap]), f"{what}: wrote between the tensors"
        if p16_on:  # the bf16 copy: a pure cast of the stored parameter, nothing outside the tensors
            assert torch.equal(p16.t[idx], p.t[idx].to(BF)), what
            assert bool(torch.isnan(p16.t[gap]).all()), what
            p16.check(what)
    for k in ("m", "v", "u", "p"):
        print(f"lamb_step {k}[{dev}] clamp-{clamp}: max err/bound so far = {RATIOS.get(f'lamb_step {k}[{dev}]', 0.0):.4f}")


# ---------------------------------------------------------------------------------------------
# 2. fused EMA
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ema_hyper_on", [False, True])
@devices
def test_lamb_step_ema(dev, ema_hyper_on):
    """The ``ema=`` variant leaves p, m, v (and the u in g) bit-identical to the plain call, and the
    average bit-identical to ``K.ema_update`` run afterwards on the stored parameters."""
    offs, off, ln, ad, total, idx, gap, w0, g0, m0, v0 = _state(dev, seed=22)
    e0 = randn(gen(dev, 23), total)
    omd = 1.0 - 0.9
    ema_hyper = torch.tensor([omd], device=dev) if ema_hyper_on else None
    kw = dict(lr=1e-2, beta1=B1, beta2=B2, eps=1e-8, weight_decay=1e-2, step=3, trust_max=10.0, grad_scale=0.5,
              max_len=max(LENS))
    outs = []
    for fused in (False, True):
        p, g, m, v = (G(total, F32, dev, init=x) for x in (w0, g0, m0, v0))
        e = G(total, F32, dev, init=e0)
        ekw = dict(ema=e.t, ema_hyper=ema_hyper, ema_one_minus_decay=(7.0 if ema_hyper_on else omd)) if fused else {}
        K.lamb_step(p.t, g.t, m.t, v.t, off, ln, ad, norms_buf(len(LENS), dev), None, **kw, **ekw)
        for b in (p, g, m, v, e):
            b.check(f"fused{int(fused)}")
        outs.append((p.t, g.t, m.t, v.t, e.t))
    (p0, u0, m_0, v_0, e_plain), (p1, u1, m_1, v_1, e_fused) = outs
    assert torch.equal(p0, p1) and torch.equal(u0, u1) and torch.equal(m_0, m_1) and torch.equal(v_0, v_1)
    assert torch.equal(e_plain, e0)  # the plain call has no average to touch
    want = e0.clone()
    K.ema_update(want, p1, one_minus_decay=(7.0 if ema_hyper_on else omd), hyper=ema_hyper)
    assert torch.equal(e_fused[idx], want[idx])
    assert torch.equal(e_fused[gap], e0[gap])  # nothing between the tensors
    assert not torch.equal(e_fused[idx], e0[idx])


# ---------------------------------------------------------------------------------------------
# 3. reproducibility
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", GPU_ONLY)
def test_lamb_step_bit_reproducible(dev):
    """Per-(tensor, block) partial sums added in fixed block order: three runs, identical bits in p and norms."""
    lens = [300000, 4096, 65548]
    offs, off, ln, ad, total = table(lens, [1, 0, 1], dev)
    g = gen(dev, 24)
    w0, g0, m0, v0 = randn(g, total), randn(g, total), randn(g, total), rand(g, total, lo=0.01, hi=2.0)
    outs = []
    for _ in range(3):
        p, gr, m, v = w0.clone(), g0.clone(), m0.clone(), v0.clone()
        norms = norms_buf(3, dev)
        K.lamb_step(p, gr, m, v, off, ln, ad, norms, None, lr=1e-2, beta1=B1, beta2=B2, eps=1e-8, weight_decay=1e-2,
                    step=2, grad_scale=0.25, max_len=max(lens))
        outs.append((p, norms))
    assert float(outs[0][1].abs().sum()) > 0
    for p, nm in outs[1:]:
        assert torch.equal(p, outs[0][0]) and torch.equal(nm, outs[0][1])


# ---------------------------------------------------------------------------------------------
# 4. wrapper refusals
# ---------------------------------------------------------------------------------------------
@devices
def test_lamb_step_refusals(dev):
    n = 64
    it = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)  # noqa: E731
    kw = dict(lr=1e-3, beta1=B1, beta2=B2, eps=1e-8, weight_decay=0.0, step=1, max_len=16)

    def call(p=None, g=None, m=None, v=None, off=None, ln=None, ad=None, norms=None, p16=None):
        z = lambda: torch.zeros(n, device=dev)  # noqa: E731
        K.lamb_step(p if p is not None else z(), g if g is not None else z(), m if m is not None else z(),
                    v if v is not None else torch.ones(n, device=dev), off if off is not None else it([0, 16]),
                    ln if ln is not None else it([16, 10]), ad if ad is not None else it([1, 0]),
                    norms if norms is not None else norms_buf(2, dev), p16, **kw)

    call()  # the base case is accepted
    with pytest.raises(ValueError, match="multiple of 4"):
        call(off=it([0, 18]))
    with pytest.raises(ValueError, match="outside"):
        call(off=it([0, 60]))
    with pytest.raises(TypeError):
        call(g=torch.zeros(n, device=dev, dtype=F64))
    with pytest.raises(TypeError):
        call(off=torch.tensor([0, 16], device=dev))  # int64 table
    with pytest.raises(TypeError):
        call(p16=torch.zeros(n, device=dev))
    with pytest.raises(ValueError):
        call(m=torch.zeros(n - 1, device=dev))
    with pytest.raises(ValueError):
        call(ln=it([16]))
    with pytest.raises(ValueError):
        call(norms=torch.zeros(K.LARS_MAX_BLOCKS * 2 * 2 - 1, dtype=F64, device=dev))
    with pytest.raises(TypeError):
        call(norms=torch.zeros(K.LARS_MAX_BLOCKS * 2 * 2, device=dev))


# ---------------------------------------------------------------------------------------------
# 5. the torch LAMB class
# ---------------------------------------------------------------------------------------------
SHAPES = [(64, 3, 7, 7), (64,), (64,), (256, 64, 1, 1), (256,), (10, 512), (10,), (5,)]


@pytest.mark.parametrize("adapt_1d", [False, True])
def test_lamb_class_matches_reference(adapt_1d):
    lens = [int(torch.tensor(s).prod()) for s in SHAPES]
    offs, off, ln, ad, total = table(lens, [int(len(s) > 1 or adapt_1d) for s in SHAPES], "cpu")
    g = gen("cpu", 25)
    p = randn(g, total)
    params = [torch.nn.Parameter(p[o:o + n].clone().view(s)) for o, n, s in zip(offs, lens, SHAPES)]
    hp = dict(lr=1e-2, eps=1e-6, weight_decay=1e-2, trust_min=0.01, trust_max=10.0)
    opt = LAMB(params, betas=(B1, B2), adapt_1d=adapt_1d, **hp)
    m, v = torch.zeros(total), torch.zeros(total)
    for step in (1, 2, 3):
        gr = randn(g, total, scale=0.1)
        for q, o, n in zip(params, offs, lens):
            q.grad = (gr[o:o + n] * 0.5).view(q.shape).clone()
        opt.step()
        R.lamb_step(p, gr, m, v, off, ln, ad, norms_buf(len(SHAPES), "cpu"), lr=hp["lr"], beta1=B1, beta2=B2,
                    eps=hp["eps"], weight_decay=hp["weight_decay"], step=step, trust_min=hp["trust_min"],
                    trust_max=hp["trust_max"], grad_scale=0.5, max_len=max(lens))
        for q, o, n in zip(params, offs, lens):
            assert torch.allclose(q.detach().reshape(-1), p[o:o + n], atol=1e-6, rtol=1e-5), (step, tuple(q.shape))
    # the reference leaves the two squared norms of tensor s in norms[2s], norms[2s + 1] and u in g
    nm = norms_buf(len(SHAPES), "cpu")
    gr, p2 = randn(g, total, scale=0.1), p.clone()
    R.lamb_step(p2, gr, m, v, off, ln, ad, nm, lr=1e-2, beta1=B1, beta2=B2, eps=1e-6, weight_decay=0.0, step=4,
                max_len=max(lens))
    for s, (o, n) in enumerate(zip(offs, lens)):
        assert torch.allclose(nm[2 * s], (p[o:o + n].double() ** 2).sum())
        assert torch.allclose(nm[2 * s + 1], (gr[o:o + n].double() ** 2).sum())


def test_build_torch_optimizer_lamb():
    q = [torch.nn.Parameter(torch.randn(4, 3)), torch.nn.Parameter(torch.randn(4))]
    oc = OptimConfig(name="lamb", lr=3e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.02, adapt_1d=True, trust_min=0.5,
                     trust_max=2.0)
    opt = build_torch_optimizer(q, oc)
    assert isinstance(opt, LAMB)
    d = opt.param_groups[0]
    assert (d["lr"], d["betas"], d["eps"], d["weight_decay"], d["adapt_1d"], d["trust_min"], d["trust_max"]) == \
        (3e-3, (0.8, 0.99), 1e-6, 0.02, True, 0.5, 2.0)


# ---------------------------------------------------------------------------------------------
# 6. trainer plumbing
# ---------------------------------------------------------------------------------------------
def _batch(batch, size, classes, seed, dev):
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (batch, size, size, 3), dtype=torch.uint8, generator=g).to(dev)
    lab = torch.randint(0, classes, (batch,), generator=g).to(dev)
    return img, lab


@pytest.mark.parametrize("adapt_1d", [False, True])
@pytest.mark.parametrize("clip", [0.0, 0.5])
@devices
def test_trainer_step_matches_oracle(dev, clip, adapt_1d):
    """Two consecutive eager LAMB steps of the native trainer on ResNet-18 against the float64 oracle
    applied per ``param_ranges`` entry to the step's own gradient (harvested from a twin trainer with
    sgd, lr = 0 on the same master and batch; the program is bit-reproducible). Pins the name-based adapt
    mask (here: the model's own ``ndim > 1``), the bias corrections and the clip pointer."""
    d = torch.device(dev if dev == "cpu" else "cuda:0")
    torch.manual_seed(0)
    model = build_model("resnet18", num_classes=10)
    ndim = {k: q.ndim for k, q in model.named_parameters()}
    twin = copy.deepcopy(model)
    lr, wd, eps = 2e-3, 1e-2, 1e-8
    A = NativeTrainer(model, 16, (32, 32), d, use_graphs=False,
                      optim=OptimConfig(name="lamb", lr=lr, weight_decay=wd, eps=eps, grad_clip=clip, adapt_1d=adapt_1d))
    Bt = NativeTrainer(twin, 16, (32, 32), d, use_graphs=False,
                       optim=OptimConfig(name="sgd", lr=0.0, momentum=0.0, weight_decay=0.0))
    assert A.opt_ranges is None and A.mom2 is not None
    assert set(ndim) == {r[0] for r in A.prog.param_ranges}
    x, y = _batch(16, 32, 10, 1, d)
    key = f"trainer clip{clip} adapt_1d{int(adapt_1d)}"
    for t in (1, 2):
        w0, m0, v0 = A.prog.master.clone(), A.mom.clone(), A.mom2.clone()
        Bt.prog.master.copy_(w0)
        Bt.step(x, y)
        g = Bt.prog.grad.clone()
        assert torch.equal(Bt.prog.master, w0)
        A.step(x, y)
        gs = 1.0
        if clip:  # the factor the kernel read through the pointer, itself checked against the gradient's norm
            got = A.clip_work[2:3].clone()
            nrm = torch.sqrt((g.double() ** 2).sum())
            want = torch.clamp(f32(clip) / (nrm + f32(1e-6)), max=1.0).reshape(1)
            # (its sum of squares: fp32 chains of at most n / (1024 blocks x 256 lanes) + 1 lane terms, 6
            # shuffles and 4 waves, then exact fp64; half of that through the square root)
            chain = g.numel() // (1024 * 256) + 1 + 10
            check("trainer clip factor", dev, got, want, f32_bound(want.abs()) + 0.5 * s_rel(chain) * want, key)
            assert float(got) < 1.0  # (the clip is active: the gradient's norm is far above 0.5)
            gs = float(got.double())
        o = SimpleNamespace(lr=f32(lr), b1=f32(B1), b2=f32(B2), eps=f32(eps), wd=f32(wd), bc1=f32(1 - B1 ** t),
                            bc2=f32(1 - B2 ** t), gs=gs, tmin=0.0, tmax=0.0)
        for name, off, n in A.prog.param_ranges:
            sl = slice(off, off + n)
            r = seg_oracle(w0[sl], g[sl], m0[sl], v0[sl], adapt_1d or ndim[name] > 1, o)
            tag = f"{key} step{t} {name}"
            check("trainer m", dev, A.mom[sl], r.m, r.mb, tag + " m")
            check("trainer v", dev, A.mom2[sl], r.v, r.vb, tag + " v")
            check("trainer p", dev, A.prog.master[sl], r.p, r.pb, tag + " p")
        assert A.step_count == t
    for k in ("m", "v", "p"):
        print(f"trainer {k}[{dev}] {key}: max err/bound so far = {RATIOS.get(f'trainer {k}[{dev}]', 0.0):.4f}")


# ---------------------------------------------------------------------------------------------
# 7. graph behaviour
# ---------------------------------------------------------------------------------------------
def _lamb(lr=2e-3, **kw):
    return OptimConfig(name="lamb", lr=lr, weight_decay=1e-2, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("clip", [0.0, 0.5])
def test_graph_matches_eager_with_lr_schedule_gpu(clip):
    """Four steps (two eager warm-ups, the capture, a replay) with a changing lr: graph == eager, bit for
    bit (lr and the bias corrections are read from the device, never from capture-time host scalars)."""
    d = torch.device("cuda:0")
    torch.manual_seed(0)
    m1 = build_model("resnet18", num_classes=10)
    m2 = copy.deepcopy(m1)
    t1 = NativeTrainer(m1, 32, (32, 32), d, optim=_lamb(grad_clip=clip), use_graphs=True)
    t2 = NativeTrainer(m2, 32, (32, 32), d, optim=_lamb(grad_clip=clip), use_graphs=False)
    x, y = _batch(32, 32, 10, 5, d)
    for i in range(4):
        for t in (t1, t2):
            t.set_lr(2e-3 * 0.5 ** i)
            t.step(x, y)
        (l1, _), (l2, _) = t1.read_metrics(), t2.read_metrics()
        assert l1 == l2, (i, l1, l2)
    assert len(t1.graphs) == 1 and t1.graphs[0] is not None
    assert torch.equal(t1.prog.master, t2.prog.master)
    assert torch.equal(t1.mom, t2.mom) and torch.equal(t1.mom2, t2.mom2)


@pytest.mark.gpu
def test_grad_accum_window_gpu():
    """grad_accum = 2: the window's update is one LAMB step on the two micro-batch gradients' sum with
    grad_scale = 1/2, bit for bit; four captured windows equal four eager ones."""
    d = torch.device("cuda:0")
    torch.manual_seed(0)
    model = build_model("resnet18", num_classes=10)
    twin, m_g, m_e = copy.deepcopy(model), copy.deepcopy(model), copy.deepcopy(model)
    data = [_batch(16, 32, 10, s, d) for s in (1, 2)]
    tr = NativeTrainer(model, 16, (32, 32), d, optim=_lamb(), use_graphs=False, grad_accum=2)
    init = tr.prog.master.clone()
    th = NativeTrainer(twin, 16, (32, 32), d, optim=OptimConfig(lr=0.0, momentum=0.0, weight_decay=0.0),
                       use_graphs=False)
    gs = []
    for x, y in data:
        th.step(x, y)
        gs.append(th.prog.grad.clone())
    tr.step(*data[0])
    assert torch.equal(tr.prog.master, init)
    tr.step(*data[1])
    assert tr.step_count == 1 and tr.micro == 0
    exp, gsum, m, v = init.clone(), gs[1] + gs[0], torch.zeros_like(init), torch.zeros_like(init)
    off, ln, ad, _, mx = tr.lamb
    K.lamb_step(exp, gsum, m, v, off, ln, ad, norms_buf(off.numel(), d), None, lr=2e-3, beta1=B1, beta2=B2, eps=1e-8,
                weight_decay=1e-2, step=1, grad_scale=0.5, max_len=mx)
    assert torch.equal(tr.prog.master, exp) and torch.equal(tr.mom, m) and torch.equal(tr.mom2, v)
    tg = NativeTrainer(m_g, 16, (32, 32), d, optim=_lamb(), use_graphs=True, grad_accum=2)
    te = NativeTrainer(m_e, 16, (32, 32), d, optim=_lamb(), use_graphs=False, grad_accum=2)
    for _ in range(4):
        for x, y in data:
            tg.step(x, y)
            te.step(x, y)
    assert tg.step_count == te.step_count == 4
    assert torch.equal(tg.prog.master, te.prog.master) and not torch.equal(tg.prog.master, init)


@pytest.mark.gpu
def test_ema_follows_updates_gpu():
    """ema_decay = 0.9 inside the captured LAMB step: after every step the average is the previous one
    moved towards the new master by the standalone kernel's rule, bit for bit."""
    d = torch.device("cuda:0")
    torch.manual_seed(0)
    tr = NativeTrainer(build_model("resnet18", num_classes=10), 16, (32, 32), d, optim=_lamb(), use_graphs=True,
                       ema_decay=0.9)
    x, y = _batch(16, 32, 10, 3, d)
    assert torch.equal(tr.ema, tr.prog.master)
    for i in range(4):
        e, w = tr.ema.clone(), tr.prog.master.clone()
        tr.step(x, y)
        K.ema_update(e, tr.prog.master, one_minus_decay=1.0 - 0.9)
        assert torch.equal(tr.ema, e), i
        assert not torch.equal(tr.prog.master, w)
    assert len(tr.graphs) == 1 and tr.graphs[0] is not None


# ---------------------------------------------------------------------------------------------
# 8. the loss falls
# ---------------------------------------------------------------------------------------------
LOSS_LR = 5e-3  # picked on the CPU reference path with this very loop (see the test's docstring)


@pytest.mark.gpu
def test_native_lamb_resnet50_graph_step_gpu():
    """The captured native step with LAMB on ResNet-50, 64x64, batch 32: the loss falls over 12 steps on
    a fixed batch. lr: the same loop on the CPU reference path (NativeTrainer on torch.device('cpu')) read
    2.697 -> 0.058 at lr 1e-3, 2.697 -> 0.0072 at 5e-3 (falling at every step) and 2.697 -> 0.012 by step 7
    then back up to 0.63 at 2e-2: 5e-3, the largest of the three that stays monotonic."""
    torch.manual_seed(0)
    d = torch.device("cuda:0")
    tr = NativeTrainer(build_model("resnet50", num_classes=10), 32, (64, 64), d,
                       optim=OptimConfig(name="lamb", lr=LOSS_LR, weight_decay=1e-2), use_graphs=True)
    x, y = _batch(32, 64, 10, 2, d)
    losses = []
    for _ in range(12):
        tr.step(x, y)
        losses.append(tr.read_metrics()[0] / 32)
    assert all(l == l for l in losses) and losses[-1] < losses[0], losses


# ---------------------------------------------------------------------------------------------
# 9. refusals and configuration
# ---------------------------------------------------------------------------------------------
def test_zero_stage_refuses_lamb():
    with pytest.raises(ValueError, match="LAMB"):
        NativeTrainer(build_model("resnet18", num_classes=10), 4, (32, 32), torch.device("cpu"),
                      optim=OptimConfig(name="lamb"), use_graphs=False, zero_stage=1)


def test_sharded_optimizers_name_lamb_in_refusal():
    """parallel/zero.py and parallel/fsdp.py keep refusing it, and say which optimizer they refuse."""
    from dbx_distributed_pytorch_examples_amd.parallel.fsdp import ShardedDataParallel
    from dbx_distributed_pytorch_examples_amd.parallel.zero import SegmentedZero, ZeroShardedOptimizer
    oc = OptimConfig(name="lamb")
    z = torch.zeros(16)
    with pytest.raises(ValueError, match="'lamb'"):
        ZeroShardedOptimizer(z, z.clone(), oc)
    with pytest.raises(ValueError, match="'lamb'"):
        SegmentedZero(None, oc, [], [])
    with pytest.raises(ValueError, match="'lamb'"):
        ShardedDataParallel(torch.nn.Linear(2, 2), oc)


def test_from_deepspeed_lamb():
    from dbx_distributed_pytorch_examples_amd.config import from_deepspeed
    ds = {"train_micro_batch_size_per_gpu": 8,
          "optimizer": {"type": "Lamb", "params": {"lr": 2e-3, "betas": [0.8, 0.99], "eps": 1e-6, "weight_decay": 0.02,
                                                   "max_coeff": 0.5, "min_coeff": 0.05}}}
    o = from_deepspeed(ds, world_size=1).optim
    assert (o.name, o.lr, tuple(o.betas), o.eps, o.weight_decay, o.trust_max, o.trust_min, o.adapt_1d) == \
        ("lamb", 2e-3, (0.8, 0.99), 1e-6, 0.02, 0.5, 0.05, True)
    o = from_deepspeed({"train_micro_batch_size_per_gpu": 8, "optimizer": {"type": "Lamb", "params": {"lr": 1e-3}}},
                       world_size=1).optim
    assert (o.name, o.lr, tuple(o.betas), o.eps, o.weight_decay, o.trust_max, o.trust_min, o.adapt_1d) == \
        ("lamb", 1e-3, (0.9, 0.999), 1e-8, 0.0, 10.0, 0.01, True)


def test_lamb_yaml_and_overrides():
    from dbx_distributed_pytorch_examples_amd.config import load_config
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "configs", "resnet50_imagenet_8192_lamb.yaml")
    cfg = load_config(path)
    o = cfg.optim
    assert o.name == "lamb" and cfg.batch_size == 1024 and cfg.model == "resnet50"
    assert (o.adapt_1d, o.trust_min, o.trust_max) == (False, 0.0, 0.0) and tuple(o.betas) == (0.9, 0.999)
    assert "untuned" in open(path).read().lower()
    cfg = load_config(path, overrides=["optim.adapt_1d=true", "optim.trust_max=10", "optim.trust_min=0.01"])
    o = cfg.optim
    assert (o.adapt_1d, o.trust_min, o.trust_max) == (True, 0.01, 10.0) and isinstance(o.trust_max, float)


def test_pick_engine_and_adapter_pass_lamb(monkeypatch):
    """``train()`` with a lamb config picks the native engine on a supported model (the decision, with a
    stub GPU device), and the native adapter hands every LAMB field to the trainer."""
    import numpy as np
    from dbx_distributed_pytorch_examples_amd.config import TrainConfig
    from dbx_distributed_pytorch_examples_amd.train import engine as E

    class DS:
        def __len__(self):
            return 64

        def __getitem__(self, i):
            return np.zeros((32, 32, 3), dtype=np.uint8), i % 10

    cfg = TrainConfig()
    cfg.model, cfg.num_classes, cfg.batch_size, cfg.precision = "resnet18", 10, 4, "bf16"
    cfg.data.image_size = 32
    cfg.optim.name, cfg.optim.lr, cfg.optim.adapt_1d, cfg.optim.trust_min, cfg.optim.trust_max = "lamb", 1e-3, True, 0.01, 10.0
    model = build_model("resnet18", num_classes=10)
    assert E._pick_engine(cfg, model, DS(), SimpleNamespace(type="cuda")) == "native"
    seen = {}

    class Stop(Exception):
        pass

    def fake(model, batch, hw, dev, optim=None, **kw):
        seen["optim"] = optim
        raise Stop

    import dbx_distributed_pytorch_examples_amd.engine.native_trainer as NT
    monkeypatch.setattr(NT, "NativeTrainer", fake)
    with pytest.raises(Stop):
        E._Native(cfg, model, DS(), torch.device("cpu"), 0)
    o = seen["optim"]
    assert (o.name, o.adapt_1d, o.trust_min, o.trust_max) == ("lamb", True, 0.01, 10.0)


def test_checkpoint_round_trip_restores_moments(tmp_path):
    from dbx_distributed_pytorch_examples_amd.train import engine as E
    d = torch.device("cpu")
    torch.manual_seed(0)
    model = build_model("resnet18", num_classes=10)
    fresh = copy.deepcopy(model)
    tr = NativeTrainer(model, 4, (32, 32), d, optim=_lamb(), use_graphs=False)
    x, y = _batch(4, 32, 10, 4, d)
    tr.step(x, y)
    tr.step(x, y)
    st = E._trainer_state(SimpleNamespace(tr=tr))
    assert st["kind"] == "native" and "mom2" in st
    torch.save(st, tmp_path / "tr.pt")
    tr2 = NativeTrainer(fresh, 4, (32, 32), d, optim=_lamb(), use_graphs=False)
    assert float(tr2.mom2.abs().sum()) == 0.0
    E._restore_trainer_state(SimpleNamespace(tr=tr2), torch.load(tmp_path / "tr.pt", weights_only=True))
    assert torch.equal(tr2.mom, tr.mom) and torch.equal(tr2.mom2, tr.mom2) and tr2.step_count == 2
    assert float(tr2.mom2.abs().sum()) > 0.0
    # the restored trainer continues like the original (bias corrections from the restored step count)
    tr2.prog.master.copy_(tr.prog.master)
    for bn, bn2 in zip(tr.prog.bns, tr2.prog.bns):
        bn2.mod.running_mean.copy_(bn.mod.running_mean)
        bn2.mod.running_var.copy_(bn.mod.running_var)
    tr.step(x, y)
    tr2.step(x, y)
    assert torch.equal(tr2.prog.master, tr.prog.master)
