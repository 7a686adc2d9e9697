"""``K.optim_step`` (the one SGD / Adam dispatch of the trainers) and the merged ``sgd`` / ``adam`` entry points.

``optim_step`` is plain Python over ``K.sgd_step`` / ``K.adam_step``: it must pass exactly what a caller who
spells every keyword out passes, so its outputs are compared bit for bit (``torch.equal``, no tolerance) with
that call, on the CPU (``ops/reference.py``) and on the GPU (``sgd_kernel`` / ``adam_kernel`` in all four
<EMA, GROUPS> instantiations). n = 1027: 256 full vectors and a 3-element scalar tail, so both paths of
``sgd_kernel`` run; with the table, the slice sits at ``run_base = 8`` of a 1035-element buffer whose last run
starts at flat index 1032 -- the tail is that run alone, and the table ends with it.

The entry points take the run table as nullable extras since they were merged; what the grouped entry points
refused (no runs, a misaligned ``run_base``, a table together with a scalar weight decay) must still be
refused before anything is launched.
"""
import itertools

import pytest
import torch

from dbx_distributed_pytorch_examples_amd.engine.native_trainer import OptimConfig
from dbx_distributed_pytorch_examples_amd.ops import kernels as K
from test_nn_ops import BF, DEVICES, GPU_ONLY, gen, rand, randn

N, RUN_BASE, N_TOTAL = 1027, 8, 1035
RUNS = [(0, 1e-2, 1.0), (512, 0.0, 0.5), (1032, 5e-3, 2.5)]  # (start, wd, lr_mult)
KINDS = {"sgd": dict(name="sgd", nesterov=False), "sgd-nesterov": dict(name="sgd", nesterov=True),
         "adam": dict(name="adam"), "adamw": dict(name="adamw")}


def _state(dev):
    g = gen(dev, 41)
    p, gr, m, e = (randn(g, N) for _ in range(4))
    return p, gr, m, rand(g, N, lo=0.0, hi=2.0), e


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("kind,ema_on,runs_on", [pytest.param(k, e, r, id=f"{k}-ema{int(e)}-runs{int(r)}")
                                                 for k, e, r in itertools.product(KINDS, (False, True), (False, True))])
def test_optim_step_equals_spelled_out_call(dev, kind, ema_on, runs_on):
    o = OptimConfig(lr=0.1, momentum=0.9, weight_decay=1e-2, betas=(0.9, 0.99), eps=1e-6, **KINDS[kind])
    sgd = o.name == "sgd"
    p0, gr, m0, v0, e0 = _state(dev)
    # the device-side values differ from o's and the keywords', so a dropped pointer shows
    hyper = torch.tensor([0.05] if sgd else [0.05, 0.19, 0.0297], device=dev)
    gsp, ema_hyper = torch.tensor([0.5], device=dev), torch.tensor([0.25], device=dev)
    extra = dict(grad_scale=0.125, grad_scale_ptr=gsp, hyper=hyper)
    if ema_on:
        extra.update(ema_hyper=ema_hyper, ema_one_minus_decay=0.01)
    if runs_on:
        extra.update(weight_decay=0.0, runs=K.pack_opt_runs(RUNS, N_TOTAL, dev), run_base=RUN_BASE)

    def bufs():
        return [p0.clone(), m0.clone(), v0.clone(), torch.zeros(N, dtype=BF, device=dev), e0.clone()]

    p, m, v, p16, e = got = bufs()
    K.optim_step(o, p, gr, m, v, p16, step=3, **extra, **(dict(ema=e) if ema_on else {}))

    p, m, v, p16, e = want = bufs()
    wd = 0.0 if runs_on else 1e-2
    tab = dict(runs=extra["runs"], run_base=RUN_BASE) if runs_on else dict(runs=None, run_base=0)
    avg = dict(ema=e, ema_hyper=ema_hyper, ema_one_minus_decay=0.01) if ema_on else \
        dict(ema=None, ema_hyper=None, ema_one_minus_decay=0.0)
    if sgd:
        K.sgd_step(p, gr, m, p16, lr=0.1, momentum=0.9, dampening=0.0, weight_decay=wd, nesterov=o.nesterov,
                   first=False, grad_scale_ptr=gsp, grad_scale=0.125, hyper=hyper, **avg, **tab)
    else:
        K.adam_step(p, gr, m, v, p16, lr=0.1, beta1=0.9, beta2=0.99, eps=1e-6, weight_decay=wd,
                    decoupled=(kind == "adamw"), step=3, grad_scale_ptr=gsp, grad_scale=0.125, hyper=hyper,
                    **avg, **tab)

    for a, b, nm in zip(got, want, ("p", "m", "v", "p16", "ema")):
        assert torch.equal(a, b), f"{kind}: {nm} differs from the spelled-out call"
    assert not torch.equal(got[0], p0) and not torch.equal(got[1], m0)  # (the step did something)
    assert torch.equal(got[2], v0) == sgd and torch.equal(got[4], e0) == (not ema_on)


@pytest.mark.parametrize("dev", DEVICES)
def test_optim_step_rejects_lamb(dev):
    p, gr, m, v, _ = _state(dev)
    with pytest.raises(ValueError, match="lamb"):
        K.optim_step(OptimConfig(name="lamb"), p, gr, m, v)


@pytest.mark.parametrize("dev", GPU_ONLY)
def test_merged_entry_points_refuse_bad_tables(dev):
    """Through the raw bindings (the wrappers' own checks bypassed): every refusal comes back as an error
    and nothing was launched -- the parameters and the state keep their bits."""
    from dbx_distributed_pytorch_examples_amd.ops._ext import C, stream_ptr
    n = 8
    g = gen(dev, 42)
    p0, gr, m0 = randn(g, n), randn(g, n), randn(g, n)
    v0 = rand(g, n, lo=0.0, hi=2.0)
    tab = K.pack_opt_runs([(0, 0.0, 1.0), (4, 0.0, 0.5)], 16, dev)
    p, m, v = p0.clone(), m0.clone(), v0.clone()

    def sgd(wd, nruns, run_base):
        C().sgd(p.data_ptr(), gr.data_ptr(), m.data_ptr(), 0, n, 0, 0.1, 0.9, 0.0, wd, 0, 0, 0, 1.0, 0, 0, 0.0,
                tab.data_ptr(), nruns, run_base, stream_ptr())

    def adam(wd, nruns, run_base):
        C().adam(p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), 0, n, 0, 0.1, 0.9, 0.999, 1e-8, wd, 1, 0.1,
                 0.001, 0, 1.0, 0, 0, 0.0, tab.data_ptr(), nruns, run_base, stream_ptr())

    for call in (sgd, adam):
        for bad in ((0.0, 0, 0), (0.0, 2, 2), (0.1, 2, 0)):  # no runs; run_base = 2; a table and wd = 0.1
            with pytest.raises(RuntimeError, match="rc=-1"):
                call(*bad)
        torch.cuda.synchronize()
        assert torch.equal(p, p0) and torch.equal(m, m0) and torch.equal(v, v0)
        call(0.0, 2, 0)  # the valid call at the same arguments goes through
        torch.cuda.synchronize()
        assert not torch.equal(p, p0)
        p.copy_(p0), m.copy_(m0), v.copy_(v0)
