"""PyTorch reference implementations of every HIP kernel, with identical signatures.

``ops.kernels`` dispatches here for CPU tensors, which makes the whole native program
(``engine.program``) runnable — and testable, including the DDP bucket path over gloo — on a
host without a GPU. They are the semantic definition the HIP kernels are tested against
(tests/test_kernels_gpu.py compares the kernels to plain fp32 torch ops of the same math).
Numerics mirror the kernels: bf16 storage, fp32 accumulation, prologue output rounded to bf16.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

NSHARD = 32  # BN-statistics shards of the large steps (see kernels.NSHARD; small steps use 4: EngineConfig.nshard)
MASK_NONE, MASK_OUT, MASK_Y = 0, 1, 2


def check_channels(C: int) -> None:
    """The per-channel passes give a thread one 8-channel group of a row, at most 256 groups a row."""
    if C < 8 or C % 8 or C // 8 > 256:
        raise ValueError(f"per-channel kernels need a channel count that is a multiple of 8, at most 2048; got {C}")


def _shards(stats, C: int):
    """The statistics slab as [nshard, 2, C] (at most 32 shards, as the kernels read it)."""
    n = stats.numel() // (2 * C)
    if n < 1 or n > 32 or n * 2 * C != stats.numel():
        raise ValueError(f"statistics slab of {stats.numel()} elements is not [nshard <= 32, 2, {C}]")
    return stats.view(n, 2, C)


def _nchw(x):
    return x.permute(0, 3, 1, 2)


def _nhwc(x):
    return x.permute(0, 2, 3, 1)


def _act_in(x, in_scale, in_shift, relu_in):
    xf = x.float()
    if in_scale is not None:
        xf = xf * in_scale + in_shift
        if relu_in:
            xf = torch.relu(xf)
        xf = xf.bfloat16().float()
    return xf


def _add_stats(stats, y):
    C = y.shape[-1]
    yf = y.float().reshape(-1, C)
    st = stats.view(-1, 2, C)
    st[0, 0] += yf.sum(0)
    st[0, 1] += (yf * yf).sum(0)


def conv_fwd(x, w16, out, *, R, S, stride, pad, stats=None, in_scale=None, in_shift=None, relu_in=True, tile=None,
             tail_res=None, tail_res_scale=None, tail_res_shift=None, tail_out=None, tail_bits=None, fin=None,
             fin_in=None, fin_in_res=None):
    for f in (fin_in, fin_in_res):  # the input BNs' finalizes, done by the consumer on the GPU
        if f is not None:
            f.run()
    OC = w16.shape[0]
    IC = x.shape[-1]
    if tail_res is not None:  # previous block's output relu(bn3(x) + shortcut): bn_apply's semantics
        act = tail_out if tail_out is not None else torch.empty_like(x)
        bn_apply(x, in_scale, in_shift, act, res=tail_res, res_scale=tail_res_scale, res_shift=tail_res_shift,
                 relu=True, mbits=tail_bits)
        xf = act.float()
    else:
        xf = _act_in(x, in_scale, in_shift, relu_in)
    w = w16.float().view(OC, R, S, IC).permute(0, 3, 1, 2)
    y = _nhwc(F.conv2d(_nchw(xf), w, stride=stride, padding=pad)).bfloat16()
    out.copy_(y.reshape(out.shape))
    if stats is not None:
        _add_stats(stats, out)
        if fin is not None:  # the kernels' in-launch BN finalize, as its own step
            fin.run()
    return out


def conv_dgrad(dy, wt16, dx, *, R, S, stride, pad, accumulate=False, tile=None, addsrc=None, add_sub=1,
               epilogue=None, bwd_y=None, bwd_coeff=None, dy_out=None, _fin=(0, 1)):
    if bwd_y is not None:  # the operand is the BN-backward apply of (dy, bwd_y)
        d = dy_out if dy_out is not None else torch.empty_like(dy)
        bn_bwd_apply(dy, bwd_y, bwd_coeff, d, mask_mode=MASK_NONE)
        dy = d
    N, P, Q, Kc = dy.shape
    _, H, W, Cc = dx.shape
    w = wt16.float().view(Cc, R, S, Kc).permute(3, 0, 1, 2)  # [K, C, R, S]
    g = torch.nn.grad.conv2d_input((N, Cc, H, W), w, _nchw(dy.float()), stride=stride, padding=pad)
    g = _nhwc(g).bfloat16().float()  # the kernel rounds the tile to bf16 before the epilogue
    if addsrc is not None:
        add = torch.zeros_like(g)
        add[:, ::add_sub, ::add_sub] = addsrc.float()
        g = g + add
    elif accumulate:
        g = g + dx.float()
    if epilogue is not None:
        e = epilogue
        y = e.ybn.float()
        if e.mode == MASK_OUT:
            w = 2 ** torch.arange(8, dtype=torch.int32, device=g.device)
            bits = (e.mbits.to(torch.int32).view(-1, 1) & w) != 0
            g = g * bits.reshape(g.shape)
        else:
            t = y * e.scale + e.shift
            g = g * (t > 0)
            if getattr(e, "act_out", None) is not None:
                e.act_out.copy_(torch.relu(t).bfloat16())
        g = g.bfloat16().float()
        gf = g.reshape(-1, Cc)
        st = e.stats1.view(-1, 2, Cc)
        st[0, 0] += gf.sum(0)
        st[0, 1] += (gf * ((y - e.mean1) * e.inv1).reshape(-1, Cc)).sum(0)
        if e.ybn2 is not None:
            st2 = e.stats2.view(-1, 2, Cc)
            st2[0, 0] += gf.sum(0)
            st2[0, 1] += (gf * ((e.ybn2.float() - e.mean2) * e.inv2).reshape(-1, Cc)).sum(0)
        if hasattr(e, "run_fin"):  # the kernels' in-launch BN-backward finalize, as its own step
            e.run_fin()
    dx.copy_(g.bfloat16())
    return dx


def conv_stem_fwd(x4, w16s, out, *, R=7, S=7, stride=2, pad=3, stats=None, patch=None):
    OC = w16s.shape[0]
    w = w16s.float().view(OC, 8, 8, 4)[:, :R, :S, :].permute(0, 3, 1, 2)
    y = _nhwc(F.conv2d(_nchw(x4.float()), w, stride=stride, padding=pad)).bfloat16()
    out.copy_(y)
    if stats is not None:
        _add_stats(stats, out)
    return out


def conv_wgrad(dy, x, dw, ws, *, R, S, stride, pad, in_scale=None, in_shift=None, relu_in=True, scale=1.0,
               accumulate=False, stem=False, tile=None, lds_pad=0, dma=-1, cnt=None, out_krsc=None, rounds=None,
               defer=None, cu_reserve=0):
    N, OH, OW, OC = dy.shape
    IC = x.shape[-1]
    xf = _act_in(x, in_scale, in_shift, relu_in)
    g = torch.nn.grad.conv2d_weight(_nchw(xf), (OC, IC, R, S), _nchw(dy.float()), stride=stride, padding=pad)
    g = g.permute(0, 2, 3, 1) * scale  # KRSC
    if stem and out_krsc is not None:  # the real input channels only (x is padded to 4)
        icr = out_krsc.numel() // (OC * R * S)
        out_krsc.copy_((g[..., :icr].reshape(-1) + (out_krsc if accumulate else 0)))
        return out_krsc
    if stem:
        full = torch.zeros(OC, 8, 8, 4, dtype=torch.float32, device=dy.device)
        full[:, :R, :S, :IC] = g
        g = full
    g = g.reshape(dw.shape)
    if accumulate:
        g = g + dw
    dw.copy_(g)
    return dw


def conv_dwfused(g, y3, coeff, wt16, y2, scale2, shift2, mean2, invstd2, bstats2, da, dw, ws, cus=0):
    """Fused bottleneck-conv3 backward = BN3-backward apply -> MASK_Y dgrad + weight gradient."""
    from types import SimpleNamespace
    dy = torch.empty_like(g)
    bn_bwd_apply(g, y3, coeff, dy, mask_mode=MASK_NONE)
    act = torch.relu(y2.float() * scale2 + shift2).bfloat16()
    epi = SimpleNamespace(mode=MASK_Y, ybn=y2, mean1=mean2, inv1=invstd2, stats1=bstats2, mbits=None, scale=scale2,
                          shift=shift2, ybn2=None, mean2=None, inv2=None, stats2=None, act_out=None)
    conv_dgrad(dy, wt16, da, R=1, S=1, stride=1, pad=0, epilogue=epi)
    conv_wgrad(dy, act, dw, ws, R=1, S=1, stride=1, pad=0)
    return da


def bn_finalize(stats, count, gamma, beta, eps, momentum, running_mean, running_var, scale, shift, save_mean,
                save_invstd):
    C = scale.numel()
    st = _shards(stats, C).double().sum(0)
    mean = st[0] / count
    var = (st[1] / count - mean * mean).clamp_min(0)
    invstd = 1.0 / torch.sqrt(var + eps)
    g = gamma.double() if gamma is not None else torch.ones_like(mean)
    b = beta.double() if beta is not None else torch.zeros_like(mean)
    scale.copy_((g * invstd).float())
    shift.copy_((b - mean * g * invstd).float())
    if save_mean is not None:
        save_mean.copy_(mean.float())
    if save_invstd is not None:
        save_invstd.copy_(invstd.float())
    if running_mean is not None and momentum > 0:
        unb = var * count / (count - 1) if count > 1 else var
        running_mean.mul_(1 - momentum).add_(momentum * mean.float())
        running_var.mul_(1 - momentum).add_(momentum * unb.float())


def bn_eval_coeff(gamma, beta, eps, running_mean, running_var, scale, shift):
    inv = torch.rsqrt(running_var + eps)
    g = gamma if gamma is not None else torch.ones_like(inv)
    b = beta if beta is not None else torch.zeros_like(inv)
    scale.copy_(g * inv)
    shift.copy_(b - running_mean * g * inv)


BN_EVAL_DESC_BYTES = 56  # csrc/nn_ops.hip BnEvalDesc: six addresses (int64), C (int32), eps (fp32)


def bn_eval_desc_dtype():
    import numpy as np
    return np.dtype([("ptr", np.int64, (6,)), ("C", np.int32), ("eps", np.float32)])


def bn_eval_coeff_multi(desc, nbn, max_c):
    """The table holds host addresses here: each entry is viewed in place and run through bn_eval_coeff."""
    import ctypes
    if desc.dtype != torch.uint8 or desc.numel() != BN_EVAL_DESC_BYTES * int(nbn):
        raise ValueError("bn_eval_coeff_multi: expected a uint8 [nbn, 56] table")

    def view(addr, n):
        return torch.frombuffer((ctypes.c_float * n).from_address(addr), dtype=torch.float32) if addr else None

    for row in desc.numpy().view(bn_eval_desc_dtype()):
        n = int(row["C"])
        if n <= 0:
            continue
        gamma, beta, rm, rv, scale, shift = (view(int(a), n) for a in row["ptr"])
        bn_eval_coeff(gamma, beta, float(row["eps"]), rm, rv, scale, shift)


def channel_stats(y, stats):
    check_channels(y.shape[-1])
    _add_stats(stats, y)


def bn_apply(y, scale, shift, out, *, res=None, res_scale=None, res_shift=None, relu=True, mbits=None, fin=None,
             res_fin=None):
    for fn in (fin, res_fin):  # (the kernel finalizes in-launch; here: the finalize first)
        if fn is not None:
            fn.run()
    check_channels(y.shape[-1])
    f = y.float() * scale + shift
    if res is not None:
        r = res.float()
        if res_scale is not None:
            r = r * res_scale + res_shift
        f = f + r
    if relu:
        f = torch.relu(f)
    out.copy_(f.bfloat16())
    if mbits is not None:
        b = (out.reshape(-1, 8).float() > 0).to(torch.int32)
        mbits.copy_((b * (2 ** torch.arange(8, dtype=torch.int32))).sum(1).to(torch.uint8))
    return out


MASK_NONE, MASK_OUT, MASK_Y = 0, 1, 2


def _g(dout, y, mask_mode, mref, scale, shift):
    g = dout.float()
    if mask_mode == MASK_OUT:
        g = g * (mref.float() > 0)
    elif mask_mode == MASK_Y:
        g = g * ((y.float() * scale + shift) > 0)
    return g


def bn_bwd_reduce(dout, y, mean, invstd, stats, *, mask_mode, mref=None, scale=None, shift=None):
    C = y.shape[-1]
    check_channels(C)
    g = _g(dout, y, mask_mode, mref, scale, shift).reshape(-1, C)
    xhat = ((y.float() - mean) * invstd).reshape(-1, C)
    st = stats.view(-1, 2, C)
    st[0, 0] += g.sum(0)
    st[0, 1] += (g * xhat).sum(0)


def bn_bwd_coeff(stats, count, gamma, mean, invstd, coeff, dgamma=None, dbeta=None, accumulate=False):
    C = mean.numel()
    st = _shards(stats, C).sum(0).float()
    s, q = st[0], st[1]
    g = gamma if gamma is not None else torch.ones_like(mean)
    sg, sgx = s / count, q / count
    k1 = g * invstd
    k2 = -g * invstd * invstd * sgx
    k3 = -g * invstd * sg + g * invstd * invstd * sgx * mean
    coeff.view(3, C).copy_(torch.stack([k1, k2, k3]))
    if dgamma is not None:
        dgamma.copy_(q + (dgamma if accumulate else 0))
    if dbeta is not None:
        dbeta.copy_(s + (dbeta if accumulate else 0))


def bn_bwd_apply(dout, y, coeff, dy, *, mask_mode, mref=None, scale=None, shift=None, gout=None, fin=None):
    if fin is not None:  # (the kernel finalizes the coefficients in-launch; here: the finalize first)
        fin.run()
    C = y.shape[-1]
    check_channels(C)
    g = _g(dout, y, mask_mode, mref, scale, shift)
    if gout is not None:
        gout.copy_(g.bfloat16())
    k = coeff.view(3, C)
    dy.copy_((k[0] * g + k[1] * y.float() + k[2]).bfloat16())


def bn_bwd_apply2(g, y1, coeff1, dy1, y2, coeff2, dy2, fin1=None, fin2=None):
    bn_bwd_apply(g, y1, coeff1, dy1, mask_mode=0, fin=fin1)
    bn_bwd_apply(g, y2, coeff2, dy2, mask_mode=0, fin=fin2)


def maxpool_fwd(x, out, arg, *, K=3, stride=2, pad=1, scale=None, shift=None, relu=True, ymax=None, fin=None):
    if fin is not None:
        fin.run()
    check_channels(x.shape[-1])
    f = x.float()
    if scale is not None:
        f = f * scale + shift
    if relu:
        f = torch.relu(f)
    N, H, W, C = f.shape
    _, P, Q, _ = out.shape
    fp = F.pad(_nchw(f), (pad, pad, pad, pad), value=-math.inf)
    xp = F.pad(_nchw(x.float()), (pad, pad, pad, pad))
    best = torch.full((N, C, P, Q), -math.inf, dtype=torch.float32, device=x.device)
    braw = torch.zeros((N, C, P, Q), dtype=torch.float32, device=x.device)
    bidx = torch.zeros((N, C, P, Q), dtype=torch.uint8, device=x.device)
    for r in range(K):
        for s in range(K):
            sl = (slice(None), slice(None), slice(r, r + stride * (P - 1) + 1, stride),
                  slice(s, s + stride * (Q - 1) + 1, stride))
            win = fp[sl]
            upd = win > best
            best = torch.where(upd, win, best)
            braw = torch.where(upd, xp[sl], braw)
            bidx = torch.where(upd, torch.full_like(bidx, r * K + s), bidx)
    out.copy_(_nhwc(best).bfloat16())
    arg.copy_(_nhwc(bidx))
    if ymax is not None:
        ymax.copy_(_nhwc(braw).bfloat16())


def maxpool_bwd(dout, arg, dx, *, K=3, stride=2, pad=1):
    N, H, W, C = dx.shape
    _, P, Q, _ = dout.shape
    acc = torch.zeros(N, C, H + 2 * pad, W + 2 * pad, dtype=torch.float32, device=dx.device)
    g = _nchw(dout.float())
    a = _nchw(arg)
    for r in range(K):
        for s in range(K):
            contrib = torch.where(a == r * K + s, g, torch.zeros_like(g))
            acc[:, :, r:r + stride * (P - 1) + 1:stride, s:s + stride * (Q - 1) + 1:stride] += contrib
    dx.copy_(_nhwc(acc[:, :, pad:pad + H, pad:pad + W]).bfloat16())


def _pool_g(dpool, arg, y, scale, shift, K, stride, pad):
    N, H, W, C = y.shape
    _, P, Q, _ = dpool.shape
    acc = torch.zeros(N, C, H + 2 * pad, W + 2 * pad, dtype=torch.float32, device=y.device)
    g = _nchw(dpool.float())
    a = _nchw(arg)
    for r in range(K):
        for s in range(K):
            acc[:, :, r:r + stride * (P - 1) + 1:stride, s:s + stride * (Q - 1) + 1:stride] += torch.where(
                a == r * K + s, g, torch.zeros_like(g))
    da = _nhwc(acc[:, :, pad:pad + H, pad:pad + W])
    return torch.where(y.float() * scale + shift > 0, da, torch.zeros_like(da))


def pool_bn_bwd_reduce(dpool, arg, y, scale, shift, mean, invstd, stats, *, K=3, stride=2, pad=1):
    C = y.shape[-1]
    g = _pool_g(dpool, arg, y, scale, shift, K, stride, pad).reshape(-1, C)
    xhat = ((y.float() - mean) * invstd).reshape(-1, C)
    st = stats.view(-1, 2, C)
    st[0, 0] += g.sum(0).double()
    st[0, 1] += (g * xhat).sum(0).double()


def pool_bn_bwd_apply(dpool, arg, y, scale, shift, coeff, dy, *, K=3, stride=2, pad=1):
    C = y.shape[-1]
    g = _pool_g(dpool, arg, y, scale, shift, K, stride, pad)
    k = coeff.view(3, C)
    dy.copy_((k[0] * g + k[1] * y.float() + k[2]).bfloat16())


def stem_bwd_fused(dpool, arg, y, scale, shift, coeff, x4, dw, ws, *, K=3, stride=2, pad=1, R=7, S=7,
                   conv_stride=2, conv_pad=3):
    """Fused stem backward = pool_bn_bwd_apply + the stem weight gradient."""
    dy = torch.empty_like(y)
    pool_bn_bwd_apply(dpool, arg, y, scale, shift, coeff, dy, K=K, stride=stride, pad=pad)
    conv_wgrad(dy, x4, dw, ws, R=R, S=S, stride=conv_stride, pad=conv_pad, stem=True)
    return dw


def avgpool_fwd(x, out):
    out.copy_(x.float().mean((1, 2)).bfloat16())


def avgpool_bwd(dout, dx):
    N, H, W, C = dx.shape
    dx.copy_((dout.float() / (H * W))[:, None, None, :].expand(N, H, W, C).bfloat16())


def softmax_ce(logits, labels, dlogits=None, loss_out=None, stats=None, smoothing=0.0, grad_scale=1.0,
               labels2=None, lam=None):
    B, C = logits.shape
    lf = logits.float()
    lse = torch.logsumexp(lf, 1)
    xl = lf.gather(1, labels[:, None]).squeeze(1)
    lm = float(lam.reshape(-1)[0]) if labels2 is not None else 1.0
    xl2 = lf.gather(1, labels2[:, None]).squeeze(1) if labels2 is not None else xl
    loss = (1 - smoothing) * (lm * (lse - xl) + (1 - lm) * (lse - xl2)) + smoothing * (lse - lf.mean(1))
    if loss_out is not None:
        loss_out.copy_(loss)
    if stats is not None:
        stats[0] += loss.sum()
        stats[1] += (lf.argmax(1) == labels).sum().float()
    if dlogits is not None:
        p = torch.softmax(lf, 1)
        t = torch.full_like(p, smoothing / C)
        t.scatter_add_(1, labels[:, None], torch.full((B, 1), (1 - smoothing) * lm, device=p.device))
        if labels2 is not None:
            t.scatter_add_(1, labels2[:, None], torch.full((B, 1), (1 - smoothing) * (1 - lm), device=p.device))
        dlogits.copy_(((p - t) * grad_scale / B).to(dlogits.dtype))


def check_bce_logits(logits, labels, dlogits=None, loss_out=None, stats=None, smoothing=0.0, grad_scale=1.0,
                     labels2=None, lam=None, target_threshold=None, sum_classes=False):
    """Host-side argument checks of :func:`bce_logits`, shared with the kernel front-end; returns
    (B, C, threshold as the kernel takes it: negative = none)."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2 or logits.dtype not in (torch.float32, torch.bfloat16) \
            or not logits.is_contiguous():
        raise TypeError("bce_logits: logits must be a contiguous [B, C] fp32 / bf16 matrix")
    B, C = logits.shape
    if C < 1:
        raise ValueError("bce_logits: logits need at least one class")
    if (labels2 is None) != (lam is None):
        raise ValueError("bce_logits: labels2 and lam come together")
    for t, dt, n, nm in ((labels, torch.int64, B, "labels"), (dlogits, logits.dtype, B * C, "dlogits"),
                         (loss_out, torch.float32, B, "loss_out"), (stats, torch.float64, 2, "stats"),
                         (labels2, torch.int64, B, "labels2"), (lam, torch.float32, 1, "lam")):
        if t is None and nm != "labels":
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != dt:
            raise TypeError(f"bce_logits: {nm}: expected a {dt} tensor, got {getattr(t, 'dtype', type(t))}")
        if t.numel() != n or not t.is_contiguous():
            raise ValueError(f"bce_logits: {nm}: expected {n} contiguous elements, got shape {tuple(t.shape)}")
        if t.device != logits.device:
            raise ValueError(f"bce_logits: {nm} is on {t.device}, logits on {logits.device}")
    if not 0.0 <= float(smoothing) < 1.0:
        raise ValueError(f"bce_logits: smoothing must be in [0, 1), got {smoothing}")
    if not math.isfinite(float(grad_scale)):
        raise ValueError(f"bce_logits: grad_scale must be finite, got {grad_scale}")
    if target_threshold is not None and not 0.0 <= float(target_threshold) < 1.0:
        raise ValueError(f"bce_logits: target_threshold must be in [0, 1) or None, got {target_threshold}")
    return B, C, -1.0 if target_threshold is None else float(target_threshold)


def bce_soft_targets(mixed, smoothing=0.0, target_threshold=None):
    """The BCE targets from mixed one-hot rows ``mixed`` [B, C] (``lam onehot(l) + (1 - lam) onehot(l2)``):
    label smoothing on top, ``(1 - s) mixed + s / C``, then timm's ``target_threshold``: ``t > thr ? 1 : 0``."""
    t = (1 - smoothing) * mixed + smoothing / mixed.shape[1]
    if target_threshold is not None:
        t = (t > target_threshold).to(t.dtype)
    return t


def bce_targets(labels, C, smoothing=0.0, labels2=None, lam=None, target_threshold=None, dtype=torch.float32):
    """:func:`bce_soft_targets` of the labels [B] (``labels2`` [B] + ``lam`` [1] device tensor: the MixUp / CutMix
    pair, read on the device). A label outside [0, C) matches no column: no positive class from it."""
    idx = torch.arange(C, device=labels.device)[None, :]
    mixed = (idx == labels[:, None]).to(dtype)
    if labels2 is not None:
        lm = lam.reshape(-1)[0].to(dtype)
        mixed = mixed * lm + (idx == labels2[:, None]).to(dtype) * (1 - lm)
    return bce_soft_targets(mixed, smoothing, target_threshold)


def bce_with_logits_loss(logits, targets, sum_classes=False):
    """The scalar training loss of the autograd engines on targets from :func:`bce_soft_targets`: timm's
    ``loss.sum(-1).mean()`` (``sum_classes``) or ``loss.mean()``."""
    loss = F.binary_cross_entropy_with_logits(logits.float(), targets.to(torch.float32), reduction="none")
    return loss.sum(-1).mean() if sum_classes else loss.mean()


def bce_logits(logits, labels, dlogits=None, loss_out=None, stats=None, smoothing=0.0, grad_scale=1.0,
               labels2=None, lam=None, target_threshold=None, sum_classes=False):
    """Binary cross-entropy on the logits with dlogits, on any device and without a host sync. Per row, in
    fp32: ``t`` = :func:`bce_targets`, ``l_c = max(x, 0) - x t + log1p(exp(-|x|))``, ``loss = sum_c l_c / D``
    with ``D = 1`` (``sum_classes``) or C, ``dlogits = (sigmoid(x) - t) grad_scale / (B D)``;
    ``stats`` (fp64 [2], accumulated) ``+= [sum of the row losses, rows whose argmax is the label]`` (the
    lowest index wins among equal logits; a label outside [0, C) is never correct)."""
    B, C, _ = check_bce_logits(logits, labels, dlogits, loss_out, stats, smoothing, grad_scale, labels2, lam,
                               target_threshold, sum_classes)
    x = logits.float()
    t = bce_targets(labels, C, smoothing, labels2, lam, target_threshold)
    e = torch.exp(-x.abs())
    D = 1 if sum_classes else C
    loss = (x.clamp(min=0) - x * t + torch.log1p(e)).sum(1) / D
    if loss_out is not None:
        loss_out.copy_(loss.view_as(loss_out))
    if stats is not None:
        idx = torch.arange(C, device=x.device)[None, :].expand(B, C)
        amax = torch.where(x == x.max(1, keepdim=True).values, idx, torch.full_like(idx, C)).min(1).values
        stats += torch.stack([loss.double().sum(), ((amax == labels) & (amax < C)).sum().double()])
    if dlogits is not None:
        r = 1 / (1 + e)
        sig = torch.where(x >= 0, r, e * r)
        dlogits.copy_(((sig - t) * (grad_scale / (B * D))).to(dlogits.dtype).view_as(dlogits))


def check_ce_eval(logits, labels, stats, k, nvalid=None, loss_out=None, rank_out=None):
    """Host-side argument checks of :func:`ce_eval`, shared with the kernel front-end; returns (B, C)."""
    if logits.dim() != 2 or logits.dtype not in (torch.float32, torch.bfloat16) or not logits.is_contiguous():
        raise TypeError("ce_eval: logits must be a contiguous [B, C] fp32 / bf16 matrix")
    B, C = logits.shape
    if isinstance(k, bool) or not isinstance(k, int):
        raise ValueError(f"ce_eval: k must be an int, got {k!r}")
    if not 1 <= k <= C:
        raise ValueError(f"ce_eval: k must be in [1, {C}], got {k}")
    for t, dt, n, nm in ((labels, torch.int64, B, "labels"), (stats, torch.float64, 4, "stats"),
                         (nvalid, torch.int32, 1, "nvalid"), (loss_out, torch.float32, B, "loss_out"),
                         (rank_out, torch.int32, B, "rank_out")):
        if t is None and nm not in ("labels", "stats"):
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != dt:
            raise TypeError(f"ce_eval: {nm}: expected a {dt} tensor, got {getattr(t, 'dtype', type(t))}")
        if t.numel() != n or not t.is_contiguous():
            raise ValueError(f"ce_eval: {nm}: expected {n} contiguous elements, got shape {tuple(t.shape)}")
        if t.device != logits.device:
            raise ValueError(f"ce_eval: {nm} is on {t.device}, logits on {logits.device}")
    return B, C


def ce_eval(logits, labels, stats, k, nvalid=None, loss_out=None, rank_out=None):
    """Evaluation metrics of a logits matrix, on any device and without a host sync: for a row with
    label l, ``rank = #{c : x_c > x_l} + #{c < l : x_c == x_l}`` (values compared in fp32; among equal
    values the lowest index wins, so ``rank == 0`` is :func:`softmax_ce`'s "correct") and
    ``loss = lse(x) - x_l`` in fp32. Rows at or past ``nvalid[0]`` (int32 device scalar) and rows whose
    label is outside [0, C) are ignored: rank -1, loss 0, nothing added, the label never used as an
    index. Every other row adds ``[loss, rank < 1, rank < k, 1]`` to ``stats`` (fp64 [4], accumulated,
    never zeroed here); a NaN label logit gives rank C (a miss at every k) and a NaN loss."""
    B, C = check_ce_eval(logits, labels, stats, k, nvalid, loss_out, rank_out)
    dev = logits.device
    lf = logits.float()
    valid = (labels >= 0) & (labels < C)
    if nvalid is not None:
        valid &= torch.arange(B, device=dev) < nvalid.reshape(-1)[0]
    lab = torch.where(valid, labels, torch.zeros_like(labels))[:, None]
    xl = lf.gather(1, lab)
    ahead = (lf > xl) | ((lf == xl) & (torch.arange(C, device=dev)[None, :] < lab))
    rank = torch.where(xl.squeeze(1).isnan(), torch.full_like(labels, C), ahead.sum(1))
    loss = torch.logsumexp(lf, 1) - xl.squeeze(1)
    loss = torch.where(valid, loss, torch.zeros_like(loss))
    stats += torch.stack([loss.double().sum(), (valid & (rank < 1)).sum().double(),
                          (valid & (rank < k)).sum().double(), valid.sum().double()])
    if loss_out is not None:
        loss_out.copy_(loss.view_as(loss_out))
    if rank_out is not None:
        rank_out.copy_(torch.where(valid, rank, torch.full_like(rank, -1)).view_as(rank_out))


OPT_MAX_RUNS = 1024  # csrc/optim_ops.hip kOptMaxRuns (the run table lives in LDS)


def _validate_opt_runs(starts, wds, lms, what: str = "pack_opt_runs") -> None:
    """``starts`` = start[0..nruns] (the last entry is n_total)."""
    nruns = len(starts) - 1
    if nruns < 1:
        raise ValueError(f"{what}: the run table is empty")
    if nruns > OPT_MAX_RUNS:
        raise ValueError(f"{what}: {nruns} runs, the kernels take at most {OPT_MAX_RUNS}")
    if starts[0] != 0:
        raise ValueError(f"{what}: the first run must start at 0, got {starts[0]}")
    if any(s % 4 for s in starts[:-1]):
        raise ValueError(f"{what}: every run start must be a multiple of 4 elements")
    if any(b <= a for a, b in zip(starts, starts[1:])):
        raise ValueError(f"{what}: run starts must be strictly increasing and below n_total={starts[-1]}")
    if starts[-1] >= 2 ** 31:
        raise ValueError(f"{what}: n_total={starts[-1]} does not fit the table's int32 indices")
    for nm, vals in (("weight_decay", wds), ("lr_mult", lms)):
        if any(not math.isfinite(x) or x < 0 for x in vals):
            raise ValueError(f"{what}: {nm} values must be finite and >= 0")


def pack_opt_runs(runs, n_total: int, device=None) -> torch.Tensor:
    """The run table of :func:`sgd_step` / :func:`adam_step` (``runs=``) from ``[(start, weight_decay, lr_mult)]``:
    run r covers flat indices [start[r], start[r+1]) and the last one ends at ``n_total``. Starts are strictly
    increasing multiples of 4 from 0; at most ``OPT_MAX_RUNS`` runs (merge equal neighbours first). One int32
    tensor ``start[nruns + 1] | wd[nruns] | lr_mult[nruns]`` (the last two as fp32 bits). Validated here, on
    the host: a step that uses the table never reads it back."""
    runs = [(int(s), float(w), float(m)) for s, w, m in runs]
    starts = [r[0] for r in runs] + [int(n_total)]
    wds, lms = [r[1] for r in runs], [r[2] for r in runs]
    _validate_opt_runs(starts, wds, lms)
    f = torch.tensor(wds + lms, dtype=torch.float32).view(torch.int32)
    tab = torch.cat([torch.tensor(starts, dtype=torch.int32), f]).to(device)
    tab._dbx_runs = (tab._version, starts, wds, lms)
    return tab


def check_opt_runs(tab, n: int, run_base: int, weight_decay: float, what: str):
    """Host checks of a grouped optimizer call; returns (starts, wds, lms) as host lists. The table is
    validated (and read back, unless :func:`pack_opt_runs` built it) once per tensor object and version."""
    if not isinstance(tab, torch.Tensor) or tab.dtype != torch.int32 or tab.dim() != 1 or not tab.is_contiguous() \
            or tab.numel() < 4 or (tab.numel() - 1) % 3:
        raise TypeError(f"{what}: runs must be the int32 table of pack_opt_runs")
    if float(weight_decay) != 0.0:
        raise ValueError(f"{what}: with runs the table carries the (absolute) weight decays; leave weight_decay at 0.0")
    ok = getattr(tab, "_dbx_runs", None)
    if ok is None or ok[0] != tab._version:
        nruns = (tab.numel() - 1) // 3
        host = tab.cpu()
        starts = host[:nruns + 1].tolist()
        f = host[nruns + 1:].view(torch.float32).tolist()
        _validate_opt_runs(starts, f[:nruns], f[nruns:], what)
        ok = tab._dbx_runs = (tab._version, starts, f[:nruns], f[nruns:])
    _, starts, wds, lms = ok
    run_base = int(run_base)
    if run_base % 4:
        raise ValueError(f"{what}: run_base={run_base} must be a multiple of 4 elements")
    if run_base < 0 or run_base + n > starts[-1]:
        raise ValueError(f"{what}: the table covers [0, {starts[-1]}), the slice is [{run_base}, {run_base + n})")
    return starts, wds, lms


def _expand_opt_runs(starts, vals, lo: int, hi: int, device) -> torch.Tensor:
    """One fp32 value per element of [lo, hi) (values rounded to fp32 as the device table holds them)."""
    out = torch.empty(hi - lo, dtype=torch.float32, device=device)
    for r, val in enumerate(vals):
        a, b = max(starts[r], lo), min(starts[r + 1], hi)
        if a < b:
            out[a - lo:b - lo] = val
    return out


def sgd_step(p, g, v, p16=None, *, lr, momentum, dampening=0.0, weight_decay=0.0, nesterov=False, first=False,
             grad_scale_ptr=None, grad_scale=1.0, hyper=None, ema=None, ema_hyper=None, ema_one_minus_decay=0.0,
             runs=None, run_base=0):
    if ema is not None:
        _chk_ema_pair(ema, p, "sgd_step")
    if hyper is not None:
        lr = float(hyper[0])
    if runs is not None:  # per-element fp32 wd and lr * lr_mult vectors, otherwise the plain formula
        n = p.numel()
        starts, wds, lms = check_opt_runs(runs, n, run_base, weight_decay, "sgd_step")
        weight_decay = _expand_opt_runs(starts, wds, run_base, run_base + n, p.device)
        lr = torch.tensor(lr, dtype=torch.float32) * _expand_opt_runs(starts, lms, run_base, run_base + n, p.device)
    gs = grad_scale * (float(grad_scale_ptr[0]) if grad_scale_ptr is not None else 1.0)
    d = g * gs + weight_decay * p
    if momentum != 0:
        if first:
            v.copy_(d)
        else:
            v.mul_(momentum).add_(d, alpha=1 - dampening)
        d = d + momentum * v if nesterov else v
    p.sub_(lr * d)
    if p16 is not None:
        p16.copy_(p.bfloat16())
    if ema is not None:
        ema_update(ema, p, one_minus_decay=ema_one_minus_decay, hyper=ema_hyper)


def adam_step(p, g, m, v, p16=None, *, lr, beta1, beta2, eps, weight_decay, decoupled, step, grad_scale_ptr=None,
              grad_scale=1.0, hyper=None, ema=None, ema_hyper=None, ema_one_minus_decay=0.0, runs=None, run_base=0):
    if ema is not None:
        _chk_ema_pair(ema, p, "adam_step")
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    if hyper is not None:
        lr, bc1, bc2 = float(hyper[0]), float(hyper[1]), float(hyper[2])
    shrink = None
    if runs is not None:  # per-element fp32 vectors; the decoupled factor per run, formed as the scalar one is
        n = p.numel()
        starts, wds, lms = check_opt_runs(runs, n, run_base, weight_decay, "adam_step")
        if decoupled:
            shrink = _expand_opt_runs(starts, [1 - (lr * lm) * wd for wd, lm in zip(wds, lms)], run_base,
                                      run_base + n, p.device)
        weight_decay = _expand_opt_runs(starts, wds, run_base, run_base + n, p.device)
        lr = torch.tensor(lr, dtype=torch.float32) * _expand_opt_runs(starts, lms, run_base, run_base + n, p.device)
    gs = grad_scale * (float(grad_scale_ptr[0]) if grad_scale_ptr is not None else 1.0)
    gg = g * gs
    if decoupled:
        p.mul_(shrink if shrink is not None else 1 - lr * weight_decay)
    else:
        gg = gg + weight_decay * p
    # (1 - beta as the kernel forms it, from the fp32 beta: 1 - 0.999 in double is 4.7e-5 off 1.f - 0.999f)
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))
    m.mul_(beta1).add_(gg, alpha=1 - f32(beta1))
    v.mul_(beta2).addcmul_(gg, gg, value=1 - f32(beta2))
    p.sub_(lr * (m / bc1) / (torch.sqrt(v / bc2) + eps))
    if p16 is not None:
        p16.copy_(p.bfloat16())
    if ema is not None:
        ema_update(ema, p, one_minus_decay=ema_one_minus_decay, hyper=ema_hyper)


def lars_scale(p, g, seg_off, seg_len, adapt, norms, *, grad_scale, eta, weight_decay, max_len):
    for s, (o, n, a) in enumerate(zip(seg_off.tolist(), seg_len.tolist(), adapt.tolist())):
        w, d = p[o:o + n], g[o:o + n]
        d.mul_(grad_scale)
        wn, gn = w.norm(), d.norm()
        norms[2 * s], norms[2 * s + 1] = wn * wn, gn * gn
        if a:
            trust = float(eta * wn / (gn + weight_decay * wn)) if (wn > 0 and gn > 0) else 1.0
            d.add_(w, alpha=weight_decay).mul_(trust)


def lamb_step(p, g, m, v, seg_off, seg_len, adapt, norms, p16=None, *, lr, beta1, beta2, eps, weight_decay, step,
              trust_min=0.0, trust_max=0.0, grad_scale_ptr=None, grad_scale=1.0, hyper=None, max_len, ema=None,
              ema_hyper=None, ema_one_minus_decay=0.0):
    """LAMB per segment in plain fp32 torch (the kernel's formula, see kernels.lamb_step): u is left in
    g, norms[2s], norms[2s + 1] = |w|^2, |u|^2 of segment s. Makes the wrapper's checks itself."""
    n = p.numel()
    for t, nm in ((p, "p"), (g, "g"), (m, "m"), (v, "v")):
        if t.dtype != torch.float32:
            raise TypeError(f"{nm}: expected torch.float32, got {t.dtype}")
        if t.numel() != n or not t.is_contiguous():
            raise ValueError(f"{nm}: expected {n} contiguous elements, got {t.numel()}")
    if p16 is not None:
        if p16.dtype != torch.bfloat16:
            raise TypeError(f"p16: expected torch.bfloat16, got {p16.dtype}")
        if p16.numel() != n:
            raise ValueError(f"p16: expected {n} elements, got {p16.numel()}")
    nseg = seg_off.numel()
    for t, nm in ((seg_off, "seg_off"), (seg_len, "seg_len"), (adapt, "adapt")):
        if t.dtype != torch.int32:
            raise TypeError(f"{nm}: expected torch.int32, got {t.dtype}")
        if t.numel() != nseg:
            raise ValueError(f"{nm}: expected {nseg} elements, got {t.numel()}")
    if norms.dtype != torch.float64:
        raise TypeError(f"norms: expected torch.float64, got {norms.dtype}")
    if norms.numel() != 64 * 2 * nseg:
        raise ValueError(f"norms: expected {64 * 2 * nseg} elements, got {norms.numel()}")
    offs, lens = seg_off.tolist(), seg_len.tolist()
    if any(o % 4 for o in offs):
        raise ValueError("lamb_step: every segment offset must be a multiple of 4 elements")
    if any(o < 0 or l < 0 or o + l > n for o, l in zip(offs, lens)):
        raise ValueError(f"lamb_step: a segment lies outside the {n}-element buffer")
    if ema is not None:
        _chk_ema_pair(ema, p, "lamb_step")
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    if hyper is not None:
        lr, bc1, bc2 = float(hyper[0]), float(hyper[1]), float(hyper[2])
    gs = grad_scale * (float(grad_scale_ptr[0]) if grad_scale_ptr is not None else 1.0)
    # the kernel forms 1 - b from the fp32 b (exactly): 1 - fl32(0.999) is 1.3e-5 below fl32(1 - 0.999),
    # which v shows in full on the first step (v = (1 - b2) gg^2)
    beta1, beta2 = (float(torch.tensor(b, dtype=torch.float32)) for b in (beta1, beta2))
    for s, (o, ln, a) in enumerate(zip(offs, lens, adapt.tolist())):
        w, d, mm, vv = p[o:o + ln], g[o:o + ln], m[o:o + ln], v[o:o + ln]
        gg = d * gs
        mm.mul_(beta1).add_(gg, alpha=1 - beta1)
        vv.mul_(beta2).addcmul_(gg, gg, value=1 - beta2)
        u = (mm / bc1) / (torch.sqrt(vv / bc2) + eps)
        if a:
            u = u + weight_decay * w
        d.copy_(u)
        ww, uu = (w.double() ** 2).sum(), (u.double() ** 2).sum()
        norms[2 * s], norms[2 * s + 1] = ww, uu
        t = 1.0
        if a:
            wn, un = float(torch.sqrt(ww).float()), float(torch.sqrt(uu).float())
            if wn > 0 and un > 0:
                t = float(torch.tensor(wn, dtype=torch.float32) / torch.tensor(un, dtype=torch.float32))
            if trust_min > 0:
                t = max(t, float(torch.tensor(trust_min, dtype=torch.float32)))
            if trust_max > 0:
                t = min(t, float(torch.tensor(trust_max, dtype=torch.float32)))
        w.sub_(u * float(torch.tensor(lr, dtype=torch.float32) * torch.tensor(t, dtype=torch.float32)))
        if p16 is not None:  # (like the kernel, nothing outside the segments is touched)
            p16[o:o + ln].copy_(w.bfloat16())
        if ema is not None and ln:
            ema_update(ema[o:o + ln], w, one_minus_decay=ema_one_minus_decay, hyper=ema_hyper)


def grad_accum(dst, src, *, first=False, flag=None):
    if dst.dtype != torch.float32 or src.dtype != torch.float32:
        raise TypeError("grad_accum: expected float32 tensors")
    if dst.numel() != src.numel() or not (dst.is_contiguous() and src.is_contiguous()):
        raise ValueError("grad_accum: dst and src must be contiguous with equal numel")
    if flag is not None:
        first = float(flag.reshape(-1)[0]) != 0.0
    if first:
        dst.copy_(src.view_as(dst))  # (a copy: NaN / Inf left in dst must not survive)
    else:
        dst.add_(src.view_as(dst))
    return dst


def _chk_ema_pair(e, p, what: str) -> None:
    if e.dtype != torch.float32 or p.dtype != torch.float32:
        raise TypeError(f"{what}: expected float32 tensors")
    if e.numel() != p.numel() or not (e.is_contiguous() and p.is_contiguous()):
        raise ValueError(f"{what}: the average and the parameters must be contiguous with equal numel")


def ema_update(e, p, *, one_minus_decay=0.0, hyper=None):
    """e += omd * (p - e) in fp32 with omd rounded to fp32 first: three roundings (difference, product,
    sum) where the kernel's fma has two."""
    _chk_ema_pair(e, p, "ema_update")
    omd = float(hyper.reshape(-1)[0]) if hyper is not None else float(torch.tensor(one_minus_decay, dtype=torch.float32))
    e.add_((p.view_as(e) - e) * omd)
    return e


def ema_update_multi(desc, ntensors, max_len, *, one_minus_decay=0.0, hyper=None):
    """The table holds host addresses here: each entry is viewed in place and updated like ema_update."""
    import ctypes
    if desc.dtype != torch.int64 or desc.numel() != 3 * int(ntensors):
        raise ValueError("ema_update_multi: expected an int64 [ntensors, 3] table")
    for dst, src, n in desc.reshape(-1, 3).tolist():
        if n <= 0:
            continue
        e = torch.frombuffer((ctypes.c_float * n).from_address(dst), dtype=torch.float32)
        p = torch.frombuffer((ctypes.c_float * n).from_address(src), dtype=torch.float32)
        ema_update(e, p, one_minus_decay=one_minus_decay, hyper=hyper)


def gate_scale_multi(desc, nrows, max_len, gates):
    """dst = gates[gate] * src per row, one fp32 multiply per element (the kernel's definition). The table holds
    host addresses here: each row is viewed in place; dst == src is an in-place scaling."""
    import ctypes
    if desc.dtype != torch.int64 or gates.dtype != torch.float32:
        raise TypeError("gate_scale_multi: expected an int64 table and float32 gates")
    if not 0 < int(nrows) <= 65535 or desc.numel() != 4 * int(nrows) or int(max_len) <= 0:
        raise ValueError("gate_scale_multi: expected an int64 [nrows, 4] table, 1..65535 rows, max_len > 0")
    rows = desc.reshape(-1, 4).tolist()
    g = gates.reshape(-1)
    if any(n <= 0 or n > int(max_len) or not 0 <= k < g.numel() for _, _, n, k in rows):
        raise ValueError("gate_scale_multi: a row's length or gate index is out of range")
    for dst, src, n, k in rows:
        y = torch.frombuffer((ctypes.c_float * n).from_address(dst), dtype=torch.float32)
        x = torch.frombuffer((ctypes.c_float * n).from_address(src), dtype=torch.float32)
        torch.mul(x, g[k], out=y)


def global_norm_clip_factor(g, max_norm, work):
    work.zero_()
    ss = (g.double() ** 2).sum()
    work[0:2].view(torch.float64)[0] = ss
    nrm = torch.sqrt(ss).float()
    work[2] = torch.clamp(max_norm / (nrm + 1e-6), max=1.0)
    work[3] = nrm
    return work[2:3]


def sumsq_accum(g, work):
    w = work[0:2].view(torch.float64)
    w += (g.double() ** 2).sum()


def clip_factor(work, max_norm):
    nrm = torch.sqrt(work[0:2].view(torch.float64)[0]).float()
    work[2] = torch.clamp(max_norm / (nrm + 1e-6), max=1.0)
    work[3] = nrm
    return work[2:3]


def normalize_u8(img, out, mean, std, flip=None, **kw):
    if "src" in kw or "src_channels" in kw:
        raise TypeError("normalize_u8 takes a dense batch: a ragged source is cropped and resized (augment_u8)")
    if kw:
        raise TypeError(f"normalize_u8: unexpected keyword {sorted(kw)[0]!r}")
    N, H, W, Cin = img.shape
    f = img.float() / 255.0
    if Cin == 1:
        f = f.expand(N, H, W, 3)
    if flip is not None:
        fl = flip.bool()[:, None, None, None]
        f = torch.where(fl, f.flip(2), f)
    m = torch.tensor(mean, device=img.device)
    s = torch.tensor(std, device=img.device)
    o = torch.zeros(N, H, W, 4, device=img.device)
    o[..., :3] = (f - m) / s
    out.copy_(o.bfloat16())


ERASE_MODES = ("const", "pixel")


def check_augment_mix(N, perm, mixbox, blend, erase, erase_mode, erase_rng):
    """The argument rules of ``augment_u8``'s mixing options (shared by the kernel wrapper and the CPU
    path); returns ``(seed, offset)`` of the pixel mode, else ``(None, None)``."""
    if erase_mode not in ERASE_MODES:
        raise ValueError(f"erase_mode must be one of {ERASE_MODES}, got {erase_mode!r}")
    if blend is not None and perm is None:
        raise ValueError("blend needs perm (the sample each one is blended with)")
    if blend is None and (perm is None) != (mixbox is None):
        raise ValueError("perm and mixbox come together")
    if mixbox is not None and perm is None:
        raise ValueError("mixbox needs perm")
    for t, dt, nm, n in ((perm, torch.int32, "perm", N), (mixbox, torch.int32, "mixbox", 4),
                         (blend, torch.float32, "blend", 1), (erase, torch.int32, "erase", 4 * N)):
        if t is None:
            continue
        if t.dtype != dt:
            raise TypeError(f"{nm}: expected {dt}, got {t.dtype}")
        if t.numel() != n:
            raise ValueError(f"{nm}: expected {n} elements, got {t.numel()} (shape {tuple(t.shape)})")
    if erase is None or erase_mode != "pixel":
        return None, None
    if erase_rng is None:
        raise ValueError('erase_mode "pixel" needs erase_rng = (seed, offset int32[1] tensor)')
    seed, offset = erase_rng
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"erase_rng: the seed must fit 64 bits, got {seed}")
    if not isinstance(offset, torch.Tensor) or offset.dtype != torch.int32 or offset.numel() != 1:
        raise TypeError("erase_rng: the offset is an int32[1] tensor (read at run time)")
    return seed, offset


def erase_noise(seed: int, offset: int, pix) -> torch.Tensor:
    """The "pixel" erase values [len(pix), 3] (fp32) of the Philox counters ``pix = (s Ho + oy) Wo + ox``:
    with words w0..w3 of counter pix, u(w) = ((w >> 8) + 1) 2^-24 in (0, 1], g(w) = (w >> 8) 2^-24 in [0, 1):
    z0 = sqrt(-2 ln u(w0)) cos(2 pi g(w1)), z1 = the same radius times sin(2 pi g(w1)),
    z2 = sqrt(-2 ln u(w2)) cos(2 pi g(w3)). Evaluated in float64 and rounded once."""
    import numpy as np
    pix = np.asarray(pix, dtype=np.uint64)
    w = [philox_u32(pix * np.uint64(4) + np.uint64(k), seed, offset) for k in range(4)]

    def u(x):
        return ((x >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24

    def g(x):
        return (x >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    r01, a01 = np.sqrt(-2.0 * np.log(u(w[0]))), 2.0 * np.pi * g(w[1])
    z = np.stack([r01 * np.cos(a01), r01 * np.sin(a01),
                  np.sqrt(-2.0 * np.log(u(w[2]))) * np.cos(2.0 * np.pi * g(w[3]))], axis=-1)
    return torch.from_numpy(z.astype(np.float32))


# ---------------------------------------------------------------------------------------------
# Ragged sources: a batch of uint8 images of different sizes is one 1-D byte arena and a table ``src`` int32
# [N, 4] = (offset / 16, H, W, stride): sample n's row y starts at byte 16 offset + y stride and holds W C pixel
# bytes (data/loader.py ``pack_layout`` writes stride = ceil16(W C) and offsets that are the running sum of
# H stride). A row of the table is unusable when its extent leaves the arena (counted in whole 16-byte units,
# as the kernels get it), H < 1, W < 1, stride < W C or stride % 16 != 0; it then reads as the row
# (0, 1, 1, 16): the arena's first pixel.
# ---------------------------------------------------------------------------------------------
RAGGED_SUBSTITUTE = (0, 1, 1, 16)


def check_ragged_src(img, src, N: int, src_channels, channels=(1, 3), what: str = "augment_u8") -> int:
    """The argument rules of ``src=`` (shared by the kernel wrappers and the CPU path); returns the arena's
    size in 16-byte units."""
    if isinstance(src_channels, bool) or not isinstance(src_channels, int) or src_channels not in channels:
        raise ValueError(f"{what}: src_channels must be one of {tuple(channels)}, got {src_channels!r}")
    if not isinstance(src, torch.Tensor) or src.dtype != torch.int32:
        raise TypeError(f"src: expected an int32 tensor [N, 4] (offset / 16, H, W, stride), got "
                        f"{getattr(src, 'dtype', type(src))}")
    if tuple(src.shape) != (N, 4) or not src.is_contiguous():
        raise ValueError(f"src: expected a contiguous table of shape ({N}, 4), got {tuple(src.shape)}")
    if not isinstance(img, torch.Tensor) or img.dtype != torch.uint8:
        raise TypeError(f"img: with src it is the uint8 arena, got {getattr(img, 'dtype', type(img))}")
    if img.dim() != 1 or not img.is_contiguous():
        raise ValueError(f"img: with src it is the 1-D contiguous arena, got shape {tuple(img.shape)}")
    if img.numel() < 16:
        raise ValueError(f"img: an arena holds at least 16 bytes, got {img.numel()}")
    if img.device != src.device:
        raise ValueError(f"src is on {src.device}, the arena on {img.device}")
    return img.numel() // 16


def ragged_rows(src, arena16: int, C: int):
    """The table's rows as the kernels read them: ``[(offset / 16, H, W, stride)]``, an unusable row replaced."""
    rows = []
    for off, H, W, rb in src.reshape(-1, 4).tolist():
        ok = off >= 0 and H >= 1 and W >= 1 and rb % 16 == 0 and rb >= W * C and off + (H * rb) // 16 <= arena16
        rows.append((off, H, W, rb) if ok else RAGGED_SUBSTITUTE)
    return rows


def ragged_views(img, src, C: int):
    """Per sample its own uint8 ``[H, W, C]`` view of the arena (row padding left out)."""
    out = []
    for off, H, W, rb in ragged_rows(src, img.numel() // 16, C):
        out.append(img[16 * off:16 * off + H * rb].view(H, rb)[:, :W * C].reshape(H, W, C))
    return out


def _sources(img, src, src_channels, N=None, channels=(1, 3), what="augment_u8"):
    """The batch as a sequence of per-sample ``[H, W, C]`` images: the dense tensor itself, or the views of a
    ragged source."""
    if src is None:
        return img
    check_ragged_src(img, src, N, src_channels, channels, what)
    return ragged_views(img, src, src_channels)


def augment_u8(img, out, boxes, mean, std, flip=None, perm=None, mixbox=None, *, blend=None, erase=None,
               erase_mode="const", erase_rng=None, src=None, src_channels=3):
    """The definition of ``kernels.augment_u8``. With ``src`` (int32 [N, 4]) ``img`` is the 1-D arena of a ragged
    source and every sample is cropped from its own ``[H, W, src_channels]`` view, boxes in its own coordinates."""
    N = out.shape[0] if src is not None else img.shape[0]
    img = _sources(img, src, src_channels, N)
    seed, offset = check_augment_mix(N, perm, mixbox, blend, erase, erase_mode, erase_rng)
    if blend is not None or erase is not None:
        # f_s per source sample (erased where erase[s] says so), then the blend, then the paste
        f = _augment_f32(img, out, boxes, mean, std, flip)
        _mix_tail(f, out, perm, mixbox, blend, erase, erase_mode, seed, offset)
        return
    if perm is not None:  # CutMix: the augmented batch, then the box pasted from sample perm[n]
        out.copy_(_augment_f32(img, out, boxes, mean, std, flip).bfloat16())
        y0, y1, x0, x1 = (int(v) for v in mixbox.tolist())
        if y0 < y1 and x0 < x1:
            plain = out.clone()
            out[:, y0:y1, x0:x1] = plain[perm.long()][:, y0:y1, x0:x1]
        return
    out.copy_(_augment_f32(img, out, boxes, mean, std, flip).bfloat16())


def _mix_tail(f, out, perm, mixbox, blend, erase, erase_mode, seed, offset):
    """``out`` from the normalised fp32 batch ``f`` by source sample: erase, then the blend, then the paste."""
    _, Ho, Wo, _ = out.shape
    if erase is not None:
        off = int(offset.reshape(-1)[0]) if offset is not None else 0
        for s, (y0, y1, x0, x1) in enumerate(erase.reshape(-1, 4).tolist()):
            y0, y1, x0, x1 = max(y0, 0), min(y1, Ho), max(x0, 0), min(x1, Wo)  # (the kernel tests positions)
            if y0 >= y1 or x0 >= x1:
                continue
            f[s, y0:y1, x0:x1] = 0.0
            if erase_mode == "pixel":
                oy = torch.arange(y0, y1).view(-1, 1)
                ox = torch.arange(x0, x1).view(1, -1)
                pix = ((s * Ho + oy) * Wo + ox).reshape(-1).numpy()
                f[s, y0:y1, x0:x1, :3] = erase_noise(seed, off, pix).view(y1 - y0, x1 - x0, 3).to(f.device)
    res = f
    if perm is not None:
        fp = f[perm.long()]
        w = blend.reshape(-1)[0] if blend is not None else None
        if w is not None and float(w) != 1.0:
            res = w * f + (1.0 - w) * fp  # fp32 throughout
        if mixbox is not None:
            y0, y1, x0, x1 = (int(v) for v in mixbox.tolist())
            if y0 < y1 and x0 < x1:
                res = res.clone()
                res[:, y0:y1, x0:x1] = fp[:, y0:y1, x0:x1]
    out.copy_(res.bfloat16())


def _augment_f32(img, out, boxes, mean, std, flip=None):
    """The normalised fp32 batch [N, Ho, Wo, 4] (pad channel 0) of ``augment_u8`` before its rounding."""
    _, Ho, Wo, _ = out.shape
    dev = img[0].device
    res = torch.zeros(len(img), Ho, Wo, 4, device=dev)
    m = torch.tensor(mean, device=dev)
    s = torch.tensor(std, device=dev)
    for n, v in enumerate(_augment_v255(img, Ho, Wo, boxes, flip)):
        res[n, ..., :3] = (v / 255.0 - m) / s
    return res


def _augment_v255(img, Ho, Wo, boxes, flip=None):
    """Per sample, the fp32 bilinear crop-resize [Ho, Wo, 3] in 0..255 (the kernels' expression ``v``). ``img``:
    a dense batch, or a sequence of per-sample [H, W, C] images (a ragged source)."""
    dev = img[0].device
    oy = torch.arange(Ho, device=dev).float()
    ox = torch.arange(Wo, device=dev).float()
    for n in range(len(img)):
        Hin, Win, Cin = img[n].shape
        by, bx, bh, bw = (float(v) for v in boxes[n])
        oxx = (Wo - 1 - ox) if (flip is not None and int(flip[n])) else ox
        sy = (by + (oy + 0.5) * bh / Ho - 0.5).clamp(0, Hin - 1)
        sx = (bx + (oxx + 0.5) * bw / Wo - 0.5).clamp(0, Win - 1)
        y0, x0 = sy.floor().long(), sx.floor().long()
        y1, x1 = (y0 + 1).clamp(max=Hin - 1), (x0 + 1).clamp(max=Win - 1)
        wy, wx = (sy - y0)[:, None, None], (sx - x0)[None, :, None]
        im = img[n].float()
        if Cin == 1:
            im = im.expand(Hin, Win, 3)
        im = im[..., :3]
        yield ((im[y0][:, x0] * (1 - wx) + im[y0][:, x1] * wx) * (1 - wy) + (im[y1][:, x0] * (1 - wx) + im[y1][:, x1] * wx) * wy)


# ---------------------------------------------------------------------------------------------
# TrivialAugmentWide (csrc/input_ops.hip): one of fourteen operations per sample on the uint8 image after
# crop / resize / flip and before normalisation, erasing and batch mixing. Everything here is integer
# or fixed-order fp32 (AutoContrast: float64) arithmetic, so the kernels match it bit for bit, and it
# matches Pillow (the library torchvision calls for these operations) bit for bit except at rotation
# coordinates within rounding of an integer.
#
# Per sample one row of eight 32-bit words (kind int32; p, a, b, c, d, e, f fp32 bits):
#   0 Identity
#   1-5 ShearX / ShearY / TranslateX / TranslateY / Rotate: the nearest-neighbour inverse affine map
#       xi = a (x + .5) + b (y + .5) + c, yi = d (x + .5) + e (y + .5) + f in fp32, every product and sum
#       rounded on its own, floor, out of the image = 0 (black before normalisation)
#   6 Brightness blend(0, v, p)   7 Color blend(L, v, p)   8 Contrast blend(mean L, v, p)
#   9 Sharpness blend(smooth, v, p)   10 Posterize p = bits   11 Solarize p = threshold
#   12 AutoContrast   13 Equalize
# ---------------------------------------------------------------------------------------------
TA_KINDS = 14
TA_NAMES = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast",
            "Sharpness", "Posterize", "Solarize", "AutoContrast", "Equalize")


TA_MAX_STAGES = 4  # operations in sequence per sample (chain_augment_u8)


def check_ta_stages(stages) -> int:
    if isinstance(stages, bool) or not isinstance(stages, int) or not 1 <= stages <= TA_MAX_STAGES:
        raise ValueError(f"stages must be an integer in 1..{TA_MAX_STAGES}, got {stages!r}")
    return stages


def ta_work_words(N: int, Ho: int, Wo: int, stages: int = 1) -> int:
    """int32 words of the pipeline's work buffer: T [N, Ho, Wo, 4] uint8 | histograms [N, 4, 256] int32 |
    lut [N, 3, 256] uint8 | mean [N] int32. A chain of ``stages`` > 1 operations (``chain_augment_u8``) holds two
    T (read and written in turn) and one histogram set per stage; lut and mean are reused."""
    stages = check_ta_stages(stages)
    return (2 if stages > 1 else 1) * N * Ho * Wo + stages * N * 1024 + N * 192 + N


def ta_work_views(work, N: int, Ho: int, Wo: int, stages: int = 1):
    """(T, hist, lut, mean) views of an int32 work buffer of at least :func:`ta_work_words` words. With
    ``stages`` > 1: T is [2, N, Ho, Wo, 4] and hist [stages, N, 4, 256] (contiguous: one memset zeroes all)."""
    if work.dtype != torch.int32:
        raise TypeError(f"work: expected torch.int32, got {work.dtype}")
    need = ta_work_words(N, Ho, Wo, stages)
    if work.numel() < need or not work.is_contiguous():
        raise ValueError(f"work: needs {need} contiguous int32 words for N={N}, {Ho}x{Wo}"
                         f"{f', {stages} stages' if stages > 1 else ''}, got {work.numel()}")
    w = work.view(-1)
    nt = 2 if stages > 1 else 1
    a = nt * N * Ho * Wo
    b = a + stages * N * 1024
    T, hist = w[:a].view(torch.uint8), w[a:b]
    T, hist = (T.view(N, Ho, Wo, 4), hist.view(N, 4, 256)) if stages == 1 else (T.view(2, N, Ho, Wo, 4),
                                                                                hist.view(stages, N, 4, 256))
    return T, hist, w[b:b + N * 192].view(torch.uint8).view(N, 3, 256), w[b + N * 192:b + N * 193]


def check_ta_ops(ops, N: int):
    if not isinstance(ops, torch.Tensor) or ops.dtype != torch.int32:
        raise TypeError(f"ops: expected an int32 tensor [N, 8] (kind, p, a..f as fp32 bits), got "
                        f"{getattr(ops, 'dtype', type(ops))}")
    if tuple(ops.shape) != (N, 8):
        raise ValueError(f"ops: expected shape ({N}, 8), got {tuple(ops.shape)}")


def _ta_sizes(N: int, **tensors):
    per = {"hist": 1024, "lut": 768, "tmean": 1}
    for nm, t in tensors.items():
        if t.numel() != N * per[nm]:
            raise ValueError(f"{nm}: expected {N * per[nm]} elements for {N} samples, got {t.numel()}")


def ta_luma(rgb):
    """Pillow's L of a numpy integer [..., 3] array."""
    import numpy as np
    a = np.asarray(rgb).astype(np.int64)
    return (a[..., 0] * 19595 + a[..., 1] * 38470 + a[..., 2] * 7471 + 0x8000) >> 16


def ta_pack(rgb) -> torch.Tensor:
    """uint8 [..., 3] -> the pipeline's image T, uint8 [..., 4] = (R, G, B, L)."""
    import numpy as np
    a = rgb.cpu().numpy() if isinstance(rgb, torch.Tensor) else np.asarray(rgb)
    return torch.from_numpy(np.concatenate([a, ta_luma(a)[..., None].astype(np.uint8)], -1).astype(np.uint8))


def ta_histograms(T) -> torch.Tensor:
    """int32 [N, 4, 256] of T uint8 [N, Ho, Wo, 4]."""
    import numpy as np
    a = T.cpu().numpy()
    return torch.from_numpy(np.stack([np.stack([np.bincount(a[n, ..., c].ravel(), minlength=256) for c in range(4)])
                                      for n in range(a.shape[0])]).astype(np.int32))


def _ta_blend(d, v, p):
    """``t = d + p (v - d)`` in fp32 (product and sum rounded separately); truncation inside [0, 1], else
    clamped to 0..255 first (Pillow's ``Image.blend``)."""
    import numpy as np
    p = np.float32(p)
    d, v = d.astype(np.float32), v.astype(np.float32)
    t = d + p * (v - d)
    if 0.0 <= p <= 1.0:
        return t.astype(np.int64).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int64))).astype(np.uint8)


def _ta_smooth(a):
    import numpy as np
    h, w, _ = a.shape
    o = a.copy()
    if h < 3 or w < 3:
        return o
    A = a.astype(np.int64)
    S = np.zeros((h - 2, w - 2, 3), np.int64)
    for dy in range(3):
        for dx in range(3):
            S += A[dy:dy + h - 2, dx:dx + w - 2] * (5 if dy == 1 and dx == 1 else 1)
    o[1:-1, 1:-1] = (S + 6) // 13
    return o


def _ta_affine(a, co):
    import numpy as np
    h, w, _ = a.shape
    f = np.float32
    yy, xx = np.mgrid[0:h, 0:w]
    xs, ys = xx.astype(f) + f(.5), yy.astype(f) + f(.5)
    co = [f(v) for v in co]
    xi = (co[0] * xs + co[1] * ys) + co[2]
    yi = (co[3] * xs + co[4] * ys) + co[5]
    xf, yf = np.floor(xi).astype(np.int64), np.floor(yi).astype(np.int64)
    ok = (xf >= 0) & (xf < w) & (yf >= 0) & (yf < h)
    o = np.zeros_like(a)
    o[ok] = a[yf[ok], xf[ok]]
    return o


def ta_lut_mean(hist, row):
    """(lut uint8 [3, 256], mean int) of one sample from its histograms int [4, 256] and its op row (numpy
    int32 [8]): ``lut`` is the identity unless the kind is 10-13; ``mean = (2 sum L + n) // (2 n)``."""
    import numpy as np
    hist = np.asarray(hist).astype(np.int64)
    kind = min(max(int(row[0]), 0), TA_KINDS - 1)
    p = float(np.asarray(row[1:2]).view(np.float32)[0])
    x = np.arange(256, dtype=np.int64)
    lut = np.tile(x, (3, 1))
    if kind == 10:
        bits = min(max(int(p), 0), 8)
        lut[:] = x & ((0xFF << (8 - bits)) & 0xFF)
    elif kind == 11:
        lut[:] = np.where(x.astype(np.float32) < np.float32(p), x, 255 - x)
    elif kind in (12, 13):
        for c in range(3):
            nz = np.nonzero(hist[c])[0]
            if len(nz) < 2:
                continue
            lo, hi = int(nz[0]), int(nz[-1])
            if kind == 12:
                scale = 255.0 / (hi - lo)
                off = -lo * scale
                lut[c] = [min(255, max(0, int(i * scale + off))) for i in range(256)]
            else:
                step = (int(hist[c].sum()) - int(hist[c][hi])) // 255
                if step == 0:
                    continue
                n = step // 2
                for i in range(256):
                    lut[c, i] = min(255, n // step)
                    n += int(hist[c][i])
    n = int(hist[3].sum())
    mean = (2 * int((hist[3] * x).sum()) + n) // (2 * n) if n else 0
    return lut.astype(np.uint8), mean


def ta_apply_image(a, row, lut=None, mean=None):
    """One sample: numpy uint8 [H, W, 3] and its op row (numpy int32 [8]) -> the augmented uint8 [H, W, 3].
    ``lut`` / ``mean`` default to those of the image itself."""
    import numpy as np
    a = np.ascontiguousarray(a[..., :3])
    row = np.asarray(row, dtype=np.int32)
    kind = min(max(int(row[0]), 0), TA_KINDS - 1)
    par = row[1:].view(np.float32)
    if lut is None or mean is None:
        T = ta_pack(a[None])
        lut, mean = ta_lut_mean(ta_histograms(T)[0].numpy(), row)
    if kind == 0:
        return a.copy()
    if kind <= 5:
        return _ta_affine(a, par[1:7])
    if kind == 6:
        return _ta_blend(np.zeros_like(a), a, par[0])
    if kind == 7:
        return _ta_blend(np.repeat(ta_luma(a)[..., None], 3, -1), a, par[0])
    if kind == 8:
        return _ta_blend(np.full_like(a, mean), a, par[0])
    if kind == 9:
        return _ta_blend(_ta_smooth(a), a, par[0])
    return np.stack([np.asarray(lut)[c][a[..., c]] for c in range(3)], -1).astype(np.uint8)


def crop_resize_u8(img, T, hist, boxes, flip=None, *, src=None, src_channels=3):
    """T uint8 [N, Ho, Wo, 4] = (R, G, B, L) of ``u8 = (int)(v + 0.5f)`` with v the fp32 bilinear expression of
    ``augment_u8``; adds the per-sample histograms to ``hist`` int32 [N, 4, 256]. ``src``: as ``augment_u8``."""
    N, Ho, Wo, _ = T.shape
    if src is not None:
        img = _sources(img, src, src_channels, N, (3,), "crop_resize_u8")
    elif img.shape[3] != 3:
        raise ValueError(f"crop_resize_u8 takes 3-channel images, got Cin={img.shape[3]}")
    for n, v in enumerate(_augment_v255(img, Ho, Wo, boxes, flip)):
        u = (v + 0.5).to(torch.int64).clamp(0, 255).to(torch.uint8)
        T[n].copy_(ta_pack(u))
    hist.add_(ta_histograms(T).view(hist.shape))


def ta_prepare(hist, ops, lut, tmean):
    """Per sample ``lut`` uint8 [N, 3, 256] and ``tmean`` int32 [N] from the histograms and the op table."""
    N = ops.shape[0] if ops.dim() == 2 else -1
    check_ta_ops(ops, N)
    _ta_sizes(N, hist=hist, lut=lut, tmean=tmean)
    h, o = hist.view(N, 4, 256).numpy(), ops.numpy()
    for n in range(N):
        l, m = ta_lut_mean(h[n], o[n])
        lut.view(N, 3, 256)[n].copy_(torch.from_numpy(l))
        tmean.view(-1)[n] = m


def ta_apply_u8(T, out, ops, lut, tmean, mean, std, *, perm=None, mixbox=None, blend=None, erase=None,
                erase_mode="const", erase_rng=None):
    """The mixing kernel on T: per source sample the operation of ``ops``, the erase value, the
    normalisation; then the blend and the paste as in ``augment_u8``."""
    N, Ho, Wo, _ = T.shape
    check_ta_ops(ops, N)
    _ta_sizes(N, lut=lut, tmean=tmean)
    seed, offset = check_augment_mix(N, perm, mixbox, blend, erase, erase_mode, erase_rng)
    a, o = T.numpy(), ops.numpy()
    l, mn = lut.view(N, 3, 256).numpy(), tmean.view(-1).tolist()
    f = torch.zeros(N, Ho, Wo, 4)
    m, s = torch.tensor(mean), torch.tensor(std)
    for n in range(N):
        v = torch.from_numpy(ta_apply_image(a[n], o[n], l[n], mn[n])).float()
        f[n, ..., :3] = (v / 255.0 - m) / s
    _mix_tail(f, out, perm, mixbox, blend, erase, erase_mode, seed, offset)


def trivial_augment_u8(img, out, boxes, mean, std, flip, ops, work, *, perm=None, mixbox=None, blend=None,
                       erase=None, erase_mode="const", erase_rng=None, src=None, src_channels=3):
    N, Ho, Wo, _ = out.shape
    if src is not None:
        check_ragged_src(img, src, N, src_channels, (3,), "trivial_augment_u8")
    elif img.shape[3] != 3:
        raise ValueError(f"trivial_augment_u8 takes 3-channel images, got Cin={img.shape[3]}")
    check_ta_ops(ops, N)
    T, hist, lut, tmean = ta_work_views(work, N, Ho, Wo)
    hist.zero_()
    crop_resize_u8(img, T, hist, boxes, flip, src=src, src_channels=src_channels)
    ta_prepare(hist, ops, lut, tmean)
    ta_apply_u8(T, out, ops, lut, tmean, mean, std, perm=perm, mixbox=mixbox, blend=blend, erase=erase,
                erase_mode=erase_mode, erase_rng=erase_rng)


def check_ta_stage(T_in, T_out, hist_out, ops, lut, tmean):
    """The argument rules of ``ta_stage_u8`` (shared by the kernel wrapper and the CPU path); returns
    ``(N, Ho, Wo)``. ValueError: shapes that disagree, ``T_out`` overlapping ``T_in`` (the affine kinds and
    Sharpness read ``T_in`` at other rows than the one being written)."""
    for nm, t, dt in (("T_in", T_in, torch.uint8), ("T_out", T_out, torch.uint8), ("hist_out", hist_out, torch.int32),
                      ("lut", lut, torch.uint8), ("tmean", tmean, torch.int32)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt:
            raise TypeError(f"{nm}: expected a {dt} tensor, got {getattr(t, 'dtype', type(t))}")
    if T_in.dim() != 4 or T_in.shape[3] != 4 or tuple(T_out.shape) != tuple(T_in.shape):
        raise ValueError(f"T_in / T_out: expected two [N, Ho, Wo, 4] uint8 tensors of one shape, got "
                         f"{tuple(T_in.shape)} and {tuple(T_out.shape)}")
    N, Ho, Wo, _ = T_in.shape
    check_ta_ops(ops, N)
    _ta_sizes(N, hist=hist_out, lut=lut, tmean=tmean)
    a0, b0 = T_in.data_ptr(), T_out.data_ptr()
    if T_in.device == T_out.device and a0 < b0 + T_out.numel() and b0 < a0 + T_in.numel():
        raise ValueError("T_out must not alias T_in: an operation reads rows of T_in other than the one it writes")
    return N, Ho, Wo


def ta_stage_u8(T_in, T_out, hist_out, ops, lut, tmean):
    """One operation of a chain, the definition: ``T_out[n]`` = (R, G, B, L) of :func:`ta_apply_image` on
    ``T_in[n]`` with row ``ops[n]`` (``lut`` / ``tmean`` from ``ta_prepare`` on ``T_in``'s histograms); ADDS
    ``T_out``'s histograms to ``hist_out`` int32 [N, 4, 256]."""
    N, Ho, Wo = check_ta_stage(T_in, T_out, hist_out, ops, lut, tmean)
    a, o = T_in.numpy(), ops.numpy()
    l, mn = lut.view(N, 3, 256).numpy(), tmean.view(-1).tolist()
    for n in range(N):
        T_out[n].copy_(ta_pack(ta_apply_image(a[n], o[n], l[n], mn[n])))
    hist_out.add_(ta_histograms(T_out).view(hist_out.shape))


def check_chain_ops(ops, N: int) -> int:
    """The stage count K of a chain table int32 [K, N, 8] (stage-major: each stage's [N, 8] slice is a table of
    the single-operation kernels)."""
    if not isinstance(ops, torch.Tensor) or ops.dtype != torch.int32:
        raise TypeError(f"ops: expected an int32 tensor [K, N, 8] (per stage: kind, p, a..f as fp32 bits), got "
                        f"{getattr(ops, 'dtype', type(ops))}")
    if ops.dim() != 3 or tuple(ops.shape[1:]) != (N, 8) or not ops.is_contiguous():
        raise ValueError(f"ops: expected a contiguous table of shape (K, {N}, 8), got {tuple(ops.shape)}")
    if not 1 <= ops.shape[0] <= TA_MAX_STAGES:
        raise ValueError(f"ops: a chain has 1..{TA_MAX_STAGES} stages, got K={ops.shape[0]}")
    return int(ops.shape[0])


def chain_augment_u8(img, out, boxes, mean, std, flip, ops, work, *, perm=None, mixbox=None, blend=None,
                     erase=None, erase_mode="const", erase_rng=None, src=None, src_channels=3):
    N, Ho, Wo, _ = out.shape
    if src is not None:
        check_ragged_src(img, src, N, src_channels, (3,), "chain_augment_u8")
    elif img.shape[3] != 3:
        raise ValueError(f"chain_augment_u8 takes 3-channel images, got Cin={img.shape[3]}")
    Kst = check_chain_ops(ops, N)
    T, hist, lut, tmean = ta_work_views(work, N, Ho, Wo, Kst)
    T, hist = T.view(-1, N, Ho, Wo, 4), hist.view(Kst, N, 4, 256)
    hist.zero_()
    crop_resize_u8(img, T[0], hist[0], boxes, flip, src=src, src_channels=src_channels)
    for i in range(Kst - 1):
        ta_prepare(hist[i], ops[i], lut, tmean)
        ta_stage_u8(T[i & 1], T[(i + 1) & 1], hist[i + 1], ops[i], lut, tmean)
    ta_prepare(hist[Kst - 1], ops[Kst - 1], lut, tmean)
    ta_apply_u8(T[(Kst - 1) & 1], out, ops[Kst - 1], lut, tmean, mean, std, perm=perm, mixbox=mixbox, blend=blend,
                erase=erase, erase_mode=erase_mode, erase_rng=erase_rng)


def weight_prep(master, wbuf, desc_dev, nlayers):
    d = desc_dev.view(-1, 10)
    for i in range(nlayers):
        row = d[i]
        src, fwd, tr = (int(x) for x in row[:6].view(torch.int64))
        k, rs, c = int(row[6]), int(row[7]), int(row[8])
        if tr == -2:  # stem (K, R, S, C) -> (K, 8, 8, 4) zero padded
            R, S = rs >> 4, rs & 15
            o = torch.zeros(k, 8, 8, 4, dtype=torch.bfloat16, device=wbuf.device)
            o[:, :R, :S, :c] = master[src:src + k * R * S * c].float().view(k, R, S, c).bfloat16()
            wbuf[fwd:fwd + k * 256].copy_(o.reshape(-1))
            continue
        if tr < -2:  # absolute-pointer utility entries (GPU only)
            continue
        n = k * rs * c
        w = master[src:src + n].float()
        if fwd >= 0:
            wbuf[fwd:fwd + n].copy_(w.bfloat16())
        if tr >= 0:
            wbuf[tr:tr + n].copy_(w.view(k, rs, c).permute(2, 1, 0).reshape(-1).bfloat16())


def cast_f32_bf16(x, y):
    y.copy_(x.bfloat16())


# ---- classifier head (csrc/head_ops.hip) ------------------------------------------------------------
def philox_u32(idx, seed: int, offset: int):
    """Philox-4x32-10 word ``idx % 4`` of counter (idx / 4 lo, idx / 4 hi, offset, 0), key seed --
    bit-identical to head_ops.hip (numpy uint64 arithmetic)."""
    import numpy as np
    idx = np.asarray(idx, dtype=np.uint64)
    M32 = np.uint64(0xFFFFFFFF)
    c0 = (idx >> np.uint64(2)) & M32
    c1 = (idx >> np.uint64(34)) & M32
    c2 = np.full_like(idx, np.uint64(offset & 0xFFFFFFFF))
    c3 = np.zeros_like(idx)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)
        n1 = p1 & M32
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        n3 = p0 & M32
        c0, c1, c2, c3 = n0, n1, n2, n3
        k0 = (k0 + 0x9E3779B9) & 0xFFFFFFFF
        k1 = (k1 + 0xBB67AE85) & 0xFFFFFFFF
    w = idx & np.uint64(3)
    return np.where(w == 0, c0, np.where(w == 1, c1, np.where(w == 2, c2, c3)))


def dropout_mask(numel: int, p: float, seed: int, offset: int, device=None) -> torch.Tensor:
    import numpy as np
    keep = 1.0 - p
    thr = min(0xFFFFFFFF, int(round(keep * 4294967296.0)))
    u = philox_u32(np.arange(numel, dtype=np.uint64), seed, offset)
    return torch.from_numpy((u < np.uint64(thr)).astype(np.float32) / keep).to(device)


def small_gemm(A, B, out, *, ta=False, tb=False, M, N, K, alpha=1.0, bias=None, accumulate=False, dropout=None,
               ws=None):
    a = A.float().reshape(K, M).t() if ta else A.float().reshape(M, K)
    b = B.float().reshape(K, N) if tb else B.float().reshape(N, K).t()
    if dropout is not None:
        which, pd, seed, off = dropout
        src = A if which == "A" else B
        off = int(off.reshape(-1)[0]) if isinstance(off, torch.Tensor) else int(off)
        mk = dropout_mask(src.numel(), pd, int(seed), off, src.device).reshape(src.shape)
        if which == "A":
            a = (A.float() * mk).bfloat16().float().reshape(K, M).t() if ta else \
                (A.float() * mk).bfloat16().float().reshape(M, K)
        else:
            b = (B.float() * mk).bfloat16().float().reshape(K, N) if tb else \
                (B.float() * mk).bfloat16().float().reshape(N, K).t()
    r = alpha * (a @ b)
    if bias is not None:
        r = r + bias.float().reshape(1, N)
    o = out.reshape(M, N)
    if accumulate:
        r = r + o.float()
    o.copy_(r.to(out.dtype))
    return out


def colsum(x, out, accumulate=False):
    s = x.float().sum(0)
    out.copy_(out + s if accumulate else s)
    return out


def dropout(x, y, p, seed, offset):
    offset = int(offset.reshape(-1)[0]) if isinstance(offset, torch.Tensor) else int(offset)
    y.copy_((x.float() * dropout_mask(x.numel(), p, int(seed), int(offset), x.device).reshape(x.shape)).to(y.dtype))
    return y
