"""Per-element checks of ``augment_u8``'s mixing options: the MixUp blend, random erasing ("const" and
"pixel") and their combination with the CutMix paste (csrc/input_ops.hip augment_mix_u8_kernel).

The rules are those of tests/test_nn_ops.py, whose helpers are imported: every test runs on the CPU
(``ops/reference.py``, the dispatcher's CPU path) and on the GPU (the HIP kernel); the oracle is float64
torch / numpy written here; outputs start NaN-filled between guard sentinels; the largest ``err / bound``
of each test is printed.

Definition checked: with ``f_s`` the normalised value of source sample s at an output position -- the
erase value where the position lies in ``erase[s]``, so erasing happens per source sample BEFORE any
paste or blend -- ``out[n] = f_perm[n]`` inside ``mixbox`` and ``bf16(w f_n + (1 - w) f_perm[n])`` elsewhere.

Bounds: ``bf16_bound(ref, mag)`` = ``2^-8 |ref| + 2^-20 mag``.

* blend: ``mag = w mag_n + (1 - w) mag_p`` (the two samples' own chains, two products and a sum on top:
  inside the 16 fp32 roundings).
* "const": the erased value is exactly 0 (``mag = 0``), everything else bit-equal to the un-erased call.
* "pixel": ``z = sqrt(-2 ln u) cospi(2 g)`` with u, g exact in fp32 (24-bit integers times 2^-24) and
  ``mag = r = sqrt(-2 ln u)``. The precise device functions are documented at <= 1 ulp (logf), correctly
  rounded (sqrtf; -2 x is exact) and <= 2 ulp (cospif / sinpif of the exact argument 2 g), and the product
  rounds once: at most 1/2 (log, halved by the root) + 1/2 + 2 + 1/2 < 4 ulp = 2^-22 r relative to r. That is
  inside the 2^-20 r of the plain bound, so nothing is widened and there is one ratio to record.
"""
import math

import numpy as np
import pytest
import torch

from dbx_distributed_pytorch_examples_amd.ops import kernels as K
from dbx_distributed_pytorch_examples_amd.ops import reference as R
from test_nn_ops import (AUG_CASES, AUG_STAGED, BF, DEVICES, F32, GPU_ONLY, MEAN, RATIOS, STD, G, _augment_ref, _norm_ref,
                         bf16_bound, check, gen)

devices = pytest.mark.parametrize("dev", DEVICES)
N, Ho, Wo = 3, 8, 8
FLIPS = [0, 1, 1]
PERMS = [pytest.param([2, 0, 1], id="perm201"), pytest.param([0, 2, 1], id="perm021-fixed-point")]
# the three unstaged shapes of test_nn_ops (an odd row length, a row longer than 4096 bytes) and a staged one
# (96-byte rows: a multiple of 16 from a 16-byte aligned base)
CASES = AUG_CASES + [AUG_STAGED]
cases = pytest.mark.parametrize("Win,Cin,Hin,boxes", CASES)
# boxes whose source coordinates are NOT exact in fp32: only for comparing two calls bit for bit
INEXACT = [(0.3, 1.7, 7.1, 23.3), (1.1, 0.2, 5.9, 29.9), (0.0, 3.3, 8.7, 11.3)]


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    mine = sorted(k for k in RATIOS if k.startswith("augment_mix"))
    if mine:
        print("\n[test_augment_mix] largest err / bound per test and device:")
        for k in mine:
            print(f"  {k}: {RATIOS[k]:.4f}")


def i32(x, dev):
    return torch.tensor(x, dtype=torch.int32, device=dev)


def setup(dev, Win, Cin, Hin, boxes, n=N, ho=Ho, wo=Wo, flips=FLIPS):
    g = gen(dev, 20)
    img = torch.randint(0, 256, (n, Hin, Win, Cin), generator=g, device=dev, dtype=torch.uint8)
    bx = torch.tensor(boxes, dtype=F32, device=dev)
    fl = torch.tensor(flips, dtype=torch.uint8, device=dev)
    f, mag = _norm_ref(_augment_ref(img, bx, fl, ho, wo), dev)  # float64 [n, ho, wo, 3], shared by the case's calls
    return img, bx, fl, f, mag


def run(dev, img, bx, fl, ho=Ho, wo=Wo, **kw):
    out = G((img.shape[0], ho, wo, 4), BF, dev)
    K.augment_u8(img, out.t, bx, MEAN, STD, flip=fl, **kw)
    out.check()
    assert torch.equal(out.t[..., 3], torch.zeros_like(out.t[..., 3])), "the pad channel is exactly 0 in every mode"
    return out.t


def noise64(seed, offset, n, ho, wo, dev):
    """float64 Box-Muller on the four words of Philox counter pix = (s Ho + oy) Wo + ox (the integer draws
    from reference.philox_u32, the generator the head tests pin): (z, r), each [n, ho, wo, 3]."""
    pix = np.arange(n * ho * wo, dtype=np.uint64)
    w = [R.philox_u32(pix * np.uint64(4) + np.uint64(k), seed, offset).astype(np.uint64) for k in range(4)]
    u = lambda x: ((x >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24  # noqa: E731  (0, 1]
    gg = lambda x: (x >> np.uint64(8)).astype(np.float64) * 2.0 ** -24          # noqa: E731  [0, 1)
    r01, r2 = np.sqrt(-2.0 * np.log(u(w[0]))), np.sqrt(-2.0 * np.log(u(w[2])))
    z = np.stack([r01 * np.cos(math.pi * 2.0 * gg(w[1])), r01 * np.sin(math.pi * 2.0 * gg(w[1])),
                  r2 * np.cos(math.pi * 2.0 * gg(w[3]))], -1)
    r = np.stack([r01, r01, r2], -1)
    return (torch.from_numpy(z).view(n, ho, wo, 3).to(dev), torch.from_numpy(r).view(n, ho, wo, 3).to(dev))


def oracle(f, mag, perm=None, w=1.0, mixbox=None, erase=None, noise=None):
    """The definition in float64: erase per source sample, then the blend, then the paste."""
    f, mag = f.clone(), mag.clone()
    for s, (y0, y1, x0, x1) in enumerate(erase or []):
        if y0 < y1 and x0 < x1:
            f[s, y0:y1, x0:x1] = noise[0][s, y0:y1, x0:x1] if noise is not None else 0.0
            mag[s, y0:y1, x0:x1] = noise[1][s, y0:y1, x0:x1] if noise is not None else 0.0
    if perm is None:
        return f, mag
    fp, mp = f[perm.long()], mag[perm.long()]
    w = float(torch.tensor(w, dtype=F32).double())
    ref, m = w * f + (1.0 - w) * fp, w * mag + (1.0 - w) * mp
    if mixbox is not None and mixbox[0] < mixbox[1] and mixbox[2] < mixbox[3]:
        y0, y1, x0, x1 = mixbox
        ref[:, y0:y1, x0:x1], m[:, y0:y1, x0:x1] = fp[:, y0:y1, x0:x1], mp[:, y0:y1, x0:x1]
    return ref, m


def erased_mask(erase, n=N, ho=Ho, wo=Wo):
    m = torch.zeros(n, ho, wo, dtype=torch.bool)
    for s, (y0, y1, x0, x1) in enumerate(erase):
        if y0 < y1 and x0 < x1:
            m[s, y0:y1, x0:x1] = True
    return m


# ---------------------------------------------------------------------------------------------
# blend
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("perm", PERMS)
@cases
@devices
def test_blend(dev, Win, Cin, Hin, boxes, perm):
    img, bx, fl, f, mag = setup(dev, Win, Cin, Hin, boxes)
    pm = i32(perm, dev)
    plain = run(dev, img, bx, fl)
    for w in (1.0, 0.0, 0.25, 0.7):
        got = run(dev, img, bx, fl, perm=pm, blend=torch.tensor([w], dtype=F32, device=dev))
        ref, m = oracle(f, mag, pm, w)
        check("augment_mix blend", dev, got[..., :3], ref, bf16_bound(ref, m), what=f"w={w}")
        if w == 1.0:
            assert torch.equal(got, plain), "w == 1: the bits of the call without blend"


@pytest.mark.parametrize("boxes", [CASES[0].values[3], CASES[3].values[3], INEXACT], ids=["W37", "W32-staged", "inexact"])
@devices
def test_identity_options_are_bit_equal(dev, boxes):
    """w == 1 and an all-empty erase table change no bit -- also at source coordinates that are not exact
    in fp32 (where a differently contracted interpolation would show), plain and with a CutMix box."""
    Win = 37 if boxes is CASES[0].values[3] else 32
    img, bx, fl, _, _ = setup(dev, Win, 3, 9, boxes)
    pm, box = i32([2, 0, 1], dev), i32([0, 5, 3, Wo], dev)
    one = torch.ones(1, dtype=F32, device=dev)
    empty = i32([[0, 0, 0, 0], [3, 3, 0, 8], [0, 8, 5, 2]], dev)  # y1 <= y0 or x1 <= x0: not erased
    rng = (7, i32([0], dev))
    plain, cut = run(dev, img, bx, fl), run(dev, img, bx, fl, perm=pm, mixbox=box)
    assert torch.equal(run(dev, img, bx, fl, perm=pm, blend=one), plain)
    assert torch.equal(run(dev, img, bx, fl, erase=empty), plain)
    assert torch.equal(run(dev, img, bx, fl, erase=empty, erase_mode="pixel", erase_rng=rng), plain)
    assert torch.equal(run(dev, img, bx, fl, perm=pm, mixbox=box, blend=one, erase=empty), cut)


# ---------------------------------------------------------------------------------------------
# erase "const"
# ---------------------------------------------------------------------------------------------
ERASE_TABLES = [pytest.param([(0, 0, 0, 0), (0, Ho, 0, Wo), (5, 8, 6, 8)], id="empty-full-corner"),
                pytest.param([(2, 3, 4, 5), (0, 0, 0, 0), (0, Ho, 0, Wo)], id="1x1-empty-full")]


@pytest.mark.parametrize("table", ERASE_TABLES)
@cases
@devices
def test_erase_const(dev, Win, Cin, Hin, boxes, table):
    img, bx, fl, f, mag = setup(dev, Win, Cin, Hin, boxes)
    plain = run(dev, img, bx, fl)
    got = run(dev, img, bx, fl, erase=i32(table, dev))
    m = erased_mask(table).to(dev)
    assert m.any() and not m.all()
    assert bool((got[m] == 0).all()), "erased elements are exactly 0"
    assert torch.equal(got[~m], plain[~m]), "every other element is bit-equal to the un-erased call"
    ref, mg = oracle(f, mag, erase=table)
    check("augment_mix erase const", dev, got[..., :3], ref, bf16_bound(ref, mg))
    assert torch.equal(run(dev, img, bx, fl, erase=i32([(0, 0, 0, 0)] * N, dev)), plain), "an all-empty table"


# ---------------------------------------------------------------------------------------------
# erasing travels with the sample
# ---------------------------------------------------------------------------------------------
MIXBOX = [0, 5, 3, Wo]
# erase boxes that straddle the CutMix box's bottom (y = 5) and left (x = 3) edges
STRADDLE = [(3, 7, 1, 5), (0, 2, 2, 8), (4, 6, 0, 8)]


@pytest.mark.parametrize("w", [None, 0.25])
@pytest.mark.parametrize("perm", PERMS)
@cases
@devices
def test_erase_travels_with_the_sample(dev, Win, Cin, Hin, boxes, perm, w):
    img, bx, fl, f, mag = setup(dev, Win, Cin, Hin, boxes)
    pm = i32(perm, dev)
    kw = {} if w is None else {"blend": torch.tensor([w], dtype=F32, device=dev)}
    got = run(dev, img, bx, fl, perm=pm, mixbox=i32(MIXBOX, dev), erase=i32(STRADDLE, dev), **kw)
    ref, m = oracle(f, mag, pm, 1.0 if w is None else w, MIXBOX, STRADDLE)
    check("augment_mix erase travels", dev, got[..., :3], ref, bf16_bound(ref, m), what=f"w={w}")
    # inside the box a pixel is 0 exactly where the PASTED sample is erased, whatever sample n's own box says
    src = erased_mask(STRADDLE)[torch.tensor(perm)]
    inbox = torch.zeros(N, Ho, Wo, dtype=torch.bool)
    inbox[:, MIXBOX[0]:MIXBOX[1], MIXBOX[2]:MIXBOX[3]] = True
    assert bool((got[(src & inbox).to(dev)] == 0).all())


# ---------------------------------------------------------------------------------------------
# erase "pixel"
# ---------------------------------------------------------------------------------------------
SEED = 0x9E3779B97F4A7C15  # (both key words in use)


@pytest.mark.parametrize("mix", ["none", "cutmix", "blend"])
@cases
@devices
def test_erase_pixel(dev, Win, Cin, Hin, boxes, mix):
    img, bx, fl, f, mag = setup(dev, Win, Cin, Hin, boxes)
    table = [(0, Ho, 0, Wo), (5, 8, 6, 8), (3, 7, 1, 5)]
    off = i32([11], dev)
    kw = dict(erase=i32(table, dev), erase_mode="pixel", erase_rng=(SEED, off))
    pm, w, box = None, 1.0, None
    if mix != "none":
        pm, box = i32([2, 0, 1], dev), MIXBOX
        kw.update(perm=pm, mixbox=i32(MIXBOX, dev))
    if mix == "blend":
        w = 0.25
        kw["blend"] = torch.tensor([w], dtype=F32, device=dev)
    got = run(dev, img, bx, fl, **kw)
    ref, m = oracle(f, mag, pm, w, box, table, noise64(SEED, 11, N, Ho, Wo, dev))
    check("augment_mix erase pixel", dev, got[..., :3], ref, bf16_bound(ref, m), what=mix)
    assert torch.equal(run(dev, img, bx, fl, **kw), got), "the same (seed, offset): identical bits"
    if mix == "none":
        off.add_(1)  # read from memory at run time
        nxt = run(dev, img, bx, fl, **kw)
        em = erased_mask(table).to(dev)
        assert torch.equal(nxt[~em], got[~em]), "offset + 1 changes nothing outside the erased elements"
        changed = (nxt[em][..., :3] != got[em][..., :3]).float().mean()
        assert float(changed) > 0.95, f"offset + 1 redraws the erased elements ({float(changed):.3f} changed)"
        ref2, m2 = oracle(f, mag, None, 1.0, None, table, noise64(SEED, 12, N, Ho, Wo, dev))
        check("augment_mix erase pixel", dev, nxt[..., :3], ref2, bf16_bound(ref2, m2), what="offset+1")


@devices
def test_erase_pixel_statistics(dev):
    """Three 64x64 outputs fully erased: 36,864 values with |mean| <= 5 / sqrt(n), |var - 1| <= 5 sqrt(2 / n)."""
    n, hw = 3, 64
    img = torch.zeros(n, 4, 16, 3, dtype=torch.uint8, device=dev)
    bx = torch.tensor([(0.0, 0.0, 4.0, 16.0)] * n, dtype=F32, device=dev)
    got = run(dev, img, bx, None, ho=hw, wo=hw, erase=i32([(0, hw, 0, hw)] * n, dev), erase_mode="pixel",
              erase_rng=(0x1234, i32([3], dev)))
    z = got[..., :3].double().reshape(-1)
    cnt = z.numel()
    assert cnt == 36864
    mean, var = float(z.mean()), float(z.var(unbiased=False))
    print(f"augment_mix erase pixel statistics[{dev}]: mean {mean:+.4f} (limit {5 / math.sqrt(cnt):.4f}), "
          f"var - 1 {var - 1:+.4f} (limit {5 * math.sqrt(2 / cnt):.4f})")
    assert abs(mean) <= 5 / math.sqrt(cnt)
    assert abs(var - 1) <= 5 * math.sqrt(2 / cnt)


# ---------------------------------------------------------------------------------------------
# grid stride
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", GPU_ONLY)
def test_grid_stride(dev):
    """520 samples x 8 rows = 4160 rows, more than the 4096-block grid: blend, paste and erase on."""
    n, Hin, Win = 520, 4, 16
    rs = np.random.default_rng(5)
    boxes = [(0.0, 0.0, 4.0, 16.0), (-0.5, 2.25, 2.0, 8.0)] * (n // 2)
    img, bx, fl, f, mag = setup(dev, Win, 3, Hin, boxes, n=n, flips=rs.integers(0, 2, n).tolist())
    pm = i32(rs.permutation(n).tolist(), dev)
    y0, x0 = rs.integers(0, Ho, n), rs.integers(0, Wo, n)
    table = [(int(a), int(min(Ho, a + h)), int(b), int(min(Wo, b + w))) if e else (0, 0, 0, 0)
             for a, b, h, w, e in zip(y0, x0, rs.integers(1, 6, n), rs.integers(1, 6, n), rs.integers(0, 2, n))]
    got = run(dev, img, bx, fl, perm=pm, mixbox=i32(MIXBOX, dev), blend=torch.tensor([0.25], dtype=F32, device=dev),
              erase=i32(table, dev), erase_mode="pixel", erase_rng=(SEED, i32([2], dev)))
    ref, m = oracle(f, mag, pm, 0.25, MIXBOX, table, noise64(SEED, 2, n, Ho, Wo, dev))
    check("augment_mix grid stride", dev, got[..., :3], ref, bf16_bound(ref, m))


# ---------------------------------------------------------------------------------------------
# wrapper refusals
# ---------------------------------------------------------------------------------------------
@devices
def test_refusals(dev):
    img, bx, fl, _, _ = setup(dev, 32, 3, 9, CASES[3].values[3])
    out = torch.empty(N, Ho, Wo, 4, dtype=BF, device=dev)
    pm, box = i32([2, 0, 1], dev), i32(MIXBOX, dev)
    w = torch.tensor([0.5], dtype=F32, device=dev)
    er = i32([(0, 2, 0, 2)] * N, dev)
    off = i32([0], dev)

    def call(**kw):
        K.augment_u8(img, out, bx, MEAN, STD, flip=fl, **kw)

    with pytest.raises(ValueError, match="perm"):
        call(blend=w)
    with pytest.raises(ValueError, match="erase_mode"):
        call(erase=er, erase_mode="noise")
    with pytest.raises(ValueError, match="erase_rng"):
        call(erase=er, erase_mode="pixel")
    with pytest.raises(TypeError):
        call(perm=pm, blend=w.double())
    with pytest.raises(ValueError):
        call(perm=pm, blend=torch.ones(2, dtype=F32, device=dev))
    with pytest.raises(TypeError):
        call(erase=er.long())
    with pytest.raises(ValueError):
        call(erase=er[:2])
    with pytest.raises(TypeError):
        call(erase=er, erase_mode="pixel", erase_rng=(1, off.long()))
    with pytest.raises(ValueError):
        call(perm=pm)  # (as before: without blend, perm and mixbox come together)
    with pytest.raises(TypeError):
        call(perm=pm.long(), mixbox=box, blend=w)
    with pytest.raises(TypeError):
        K.augment_u8(img, out, bx, MEAN, STD, fl, pm, box, w)  # the new options are keyword-only
    call(perm=pm, mixbox=box, blend=w, erase=er, erase_mode="pixel", erase_rng=(1, off))  # (and this is accepted)
