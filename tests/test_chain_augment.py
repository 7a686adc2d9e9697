"""Per-element checks of the chained input kernels (csrc/input_ops.hip): ``ta_stage_u8`` -- one uint8 operation
between ``ta_prepare`` and ``ta_apply_u8`` -- and the composed ``chain_augment_u8``, the K operations in sequence
of RandAugment and AutoAugment.

The rules and helpers are those of tests/test_trivial_augment.py: every test runs on the CPU
(``ops/reference.py``, the dispatcher's CPU path) and on the GPU (the HIP kernel); outputs start sentinel-filled
between guards. Every comparison is bit for bit on integers -- a stage's output IS uint8, and with unit
normalisation the bf16 output of the chain is the uint8 value -- except where a MixUp blend or ImageNet mean / std
makes the output a fraction: there the float64 oracle and ``bf16_bound`` of test_augment_mix apply unchanged, the
staged value being an exact integer.
"""
import functools

import numpy as np
import pytest
import torch

from dbx_distributed_pytorch_examples_amd.engine import mix as M
from dbx_distributed_pytorch_examples_amd.ops import kernels as K
from dbx_distributed_pytorch_examples_amd.ops import reference as R
from test_augment_mix import PERMS, i32, noise64, oracle
from test_nn_ops import BF, DEVICES, F32, GPU_ONLY, MEAN, STD, G, _norm_ref, bf16_bound, check
from test_trivial_augment import CHUNKS, ERASE, FLIPS, MIXBOX, N, SEED, UNIT, definition, images, prepared, table

devices = pytest.mark.parametrize("dev", DEVICES)
chunks = pytest.mark.parametrize("ops", CHUNKS, ids=["+".join(f"{R.TA_NAMES[k]}{m:g}" for k, m in c) for c in CHUNKS])
# (8, 8): a chunk shorter than the 16 rows a block takes; (33, 20): a one-row last chunk; (24, 40) and (33, 20):
# Sharpness and the affine gathers read across a chunk boundary
STAGE_SHAPES = [(16, 16), (24, 40), (8, 8), (33, 20)]
HGUARD, HSENT = 64, 0x5A5A5A5A


class GuardedHist:
    """int32 [n, 4, 256] between sentinel guards, starting as ``init`` (default: zero, as the caller must)."""

    def __init__(self, n, dev, init=None):
        self.buf = torch.full((n * 1024 + 2 * HGUARD,), HSENT, dtype=torch.int32, device=dev)
        self.t = self.buf[HGUARD:HGUARD + n * 1024].view(n, 4, 256)
        self.t.copy_(init) if init is not None else self.t.zero_()

    def check(self):
        assert bool((self.buf[:HGUARD] == HSENT).all()) and bool((self.buf[-HGUARD:] == HSENT).all()), "wrote outside hist"


def stage(dev, T, ops, lut, tmean, prefill=None):
    n, Ho, Wo, _ = T.shape
    out, hist = G((n, Ho, Wo, 4), torch.uint8, dev), GuardedHist(n, dev, prefill)
    K.ta_stage_u8(T, out.t, hist.t, ops, lut, tmean)
    out.check()
    hist.check()
    return out.t.cpu(), hist.t.cpu()


def assert_stage(got, hist, rgb, rows, prefill=None):
    want = definition(rgb, rows)
    assert np.array_equal(got[..., :3].numpy(), want), "R, G, B: the definition's"
    assert np.array_equal(got[..., 3].numpy(), R.ta_luma(want)), "L: Pillow's gray value of the new pixel"
    hw = R.ta_histograms(got)
    assert torch.equal(hist, hw if prefill is None else hw + prefill.cpu()), "hist_out += T_out's histograms"
    assert bool((hw.sum(-1) == rgb.shape[1] * rgb.shape[2]).all())


# ---------------------------------------------------------------------------------------------
# 1. ta_stage_u8 == the definition
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["varied", "flat"])
@chunks
@pytest.mark.parametrize("Ho,Wo", STAGE_SHAPES, ids=[f"{h}x{w}" for h, w in STAGE_SHAPES])
@devices
def test_stage_every_kind_bit_for_bit(dev, Ho, Wo, ops, which):
    rgb, rows = images(Ho, Wo, which), table(ops, Ho, Wo)
    got, hist = stage(dev, *prepared(rgb, rows, dev))
    assert_stage(got, hist, rgb, rows)


@devices
def test_stage_adds_to_the_histograms(dev):
    Ho, Wo = 24, 40
    rgb, rows = images(Ho, Wo, "varied"), table([(5, 40.5), (13, 0.0), (9, 1.99)], Ho, Wo)
    pre = torch.from_numpy(np.random.default_rng(1).integers(0, 1000, (N, 4, 256)).astype(np.int32)).to(dev)
    got, hist = stage(dev, *prepared(rgb, rows, dev), prefill=pre)
    assert_stage(got, hist, rgb, rows, pre)


# ---------------------------------------------------------------------------------------------
# 2. a row wider than one tile of 1024 columns
# ---------------------------------------------------------------------------------------------
@devices
def test_stage_row_wider_than_one_tile(dev):
    Ho, Wo = 3, 1100
    rgb = np.random.default_rng(7).integers(0, 256, (3, Ho, Wo, 3)).astype(np.uint8)
    rows = table([(5, 0.1), (10, 5.0), (9, 1.99)], Ho, Wo)  # Rotate by 0.1 degrees (a row at the row ends), Posterize
    got, hist = stage(dev, *prepared(rgb, rows, dev))
    assert_stage(got, hist, rgb, rows)
    for n in range(3):  # (not vacuous: the second tile holds changed pixels)
        assert bool((got[n, :, 1024:, :3].numpy() != rgb[n, :, 1024:]).any())


# ---------------------------------------------------------------------------------------------
# 3. grid stride
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", GPU_ONLY)
def test_stage_grid_stride(dev):
    """4100 samples of 4 x 4 = 4100 row chunks, more than the 4096-block grid."""
    n, Ho, Wo = 4100, 4, 4
    rs = np.random.default_rng(5)
    rgb = rs.integers(0, 256, (n, Ho, Wo, 3)).astype(np.uint8)
    rows = M.sample_trivial_augment(rs, n, Ho, Wo)[1]
    T, hist0 = R.ta_pack(rgb), torch.zeros(n, 4, 256, dtype=torch.int32, device=dev)
    lut, tmean = torch.empty(n, 3, 256, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    ops = torch.from_numpy(rows).to(dev)
    K.ta_prepare(R.ta_histograms(T).to(dev), ops, lut, tmean)  # (pinned to the definition by test_ta_prepare)
    out = G((n, Ho, Wo, 4), torch.uint8, dev)
    K.ta_stage_u8(T.to(dev), out.t, hist0, ops, lut, tmean)
    out.check()
    l, m = lut.cpu().numpy(), tmean.cpu().tolist()
    want = np.stack([R.ta_apply_image(rgb[j], rows[j], l[j], m[j]) for j in range(n)])
    got = out.t.cpu()
    assert np.array_equal(got[..., :3].numpy(), want) and np.array_equal(got[..., 3].numpy(), R.ta_luma(want))
    assert torch.equal(hist0.cpu(), R.ta_histograms(got))


# ---------------------------------------------------------------------------------------------
# 4. the chained call
# ---------------------------------------------------------------------------------------------
# one non-trivial magnitude per kind
MAG = {0: 0.0, 1: 0.33, 2: -0.33, 3: 7.0, 4: -5.0, 5: 40.5, 6: 0.67, 7: 1.6, 8: 1.5, 9: 1.99, 10: 3.0, 11: 127.5,
       12: 0.0, 13: 0.0}
PAIRS = [(a, b) for a in range(14) for b in range(14)]
PAIRS += [(0, 0)] * (-len(PAIRS) % N)
CHAIN_SHAPES = [(16, 16), (24, 40)]
chain_shapes = pytest.mark.parametrize("Ho,Wo", CHAIN_SHAPES, ids=[f"{h}x{w}" for h, w in CHAIN_SHAPES])
# K = 3 and K = 4, each ending in an operation that reads the image's statistics (per sample: a chain of kinds)
LONG = [[(6, 11, 8), (5, 10, 12), (9, 7, 13)],
        [(1, 6, 11, 12), (10, 3, 7, 13), (11, 9, 5, 8)]]


def chain_table(kinds, Ho, Wo):
    """``kinds``: per sample a tuple of K kinds -> int32 [K, N, 8] at MAG."""
    return np.stack([np.stack([M.ta_row(ks[j], MAG[ks[j]], Ho, Wo) for ks in kinds]) for j in range(len(kinds[0]))])


def fold(rgb, rows):
    """The definition: ``reference.ta_apply_image`` folded over the stage axis of ``rows`` [K, N, 8]."""
    for stage_rows in rows:
        rgb = definition(rgb, stage_rows)
    return rgb


@functools.lru_cache(maxsize=None)
def flipped(Ho, Wo):
    """The "varied" images after the flips (what crop_resize_u8 hands the first stage; read-only)."""
    rgb = images(Ho, Wo, "varied")
    a = np.stack([c[:, ::-1] if f else c for c, f in zip(rgb, FLIPS)])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def pair_case(Ho, Wo):
    """(tables, expected outputs) of all 14 x 14 ordered pairs, three samples per call; computed once."""
    tabs = [chain_table(PAIRS[i:i + N], Ho, Wo) for i in range(0, len(PAIRS), N)]
    return tabs, [fold(flipped(Ho, Wo), t) for t in tabs]


def chained(dev, Ho, Wo, rows, norm=UNIT, extra=3, **kw):
    """``chain_augment_u8`` on the "varied" images (an identity crop box: the source pixels exactly), flipped."""
    img = torch.from_numpy(images(Ho, Wo, "varied")).to(dev)
    bx = torch.tensor([(0.0, 0.0, Ho, Wo)] * N, dtype=F32, device=dev)
    fl = torch.tensor(FLIPS, dtype=torch.uint8, device=dev)
    out = G((N, Ho, Wo, 4), BF, dev)
    words = K.ta_work_words(N, Ho, Wo, len(rows))
    work = torch.full((words + extra,), 0x5A5A5A5A, dtype=torch.int32, device=dev)  # (stale contents)
    K.chain_augment_u8(img, out.t, bx, norm[0], norm[1], fl, torch.from_numpy(np.ascontiguousarray(rows)).to(dev), work, **kw)
    out.check()
    assert bool((work[words:] == 0x5A5A5A5A).all()), "nothing past ta_work_words is written"
    assert torch.equal(out.t[..., 3], torch.zeros_like(out.t[..., 3])), "the pad channel is exactly 0"
    return out.t


@chain_shapes
@devices
def test_chain_all_ordered_pairs(dev, Ho, Wo):
    tabs, wants = pair_case(Ho, Wo)
    for t, want in zip(tabs, wants):
        got = chained(dev, Ho, Wo, t)
        assert torch.equal(got[..., :3].cpu().double(), torch.from_numpy(want.astype(np.float64))), [
            tuple(R.TA_NAMES[k] for k in t[:, n, 0]) for n in range(N)]


@pytest.mark.parametrize("kinds", LONG, ids=["K3", "K4"])
@chain_shapes
@devices
def test_chain_of_three_and_four(dev, Ho, Wo, kinds):
    t = chain_table(kinds, Ho, Wo)
    assert t.shape[0] == len(kinds[0]) and all(ks[-1] in (8, 12, 13) for ks in kinds)
    got = chained(dev, Ho, Wo, t)
    assert torch.equal(got[..., :3].cpu().double(), torch.from_numpy(fold(flipped(Ho, Wo), t).astype(np.float64)))


# ---------------------------------------------------------------------------------------------
# 5. the second stage sees the first (non-vacuity of 4.)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first,second", [(6, 8), (11, 12), (10, 13), (5, 7)],
                         ids=["Brightness-Contrast", "Solarize-AutoContrast", "Posterize-Equalize", "Rotate-Color"])
def test_stale_statistics_would_show(first, second):
    """The second operation evaluated with the FIRST image's histograms / gray mean / L differs from the
    definition on the "varied" images: a kernel that reused them fails test_chain_all_ordered_pairs. Asserted
    over that test's shapes together: Equalize's LUT from the un-posterized histogram agrees with the right one
    at every posterized level (the cumulative counts below a multiple of 32 are the same) unless the step
    ``(pixels - last bin) // 255`` changes, which it does at 16 x 16 (1 -> 0) and not at 24 x 40 (3 -> 3)."""
    assert any(_stale_differs(Ho, Wo, first, second) for Ho, Wo in CHAIN_SHAPES)


def _stale_differs(Ho, Wo, first, second):
    rgb = flipped(Ho, Wo)
    r1, r2 = M.ta_row(first, MAG[first], Ho, Wo), M.ta_row(second, MAG[second], Ho, Wo)
    differs = False
    for n in range(N):
        mid = R.ta_apply_image(rgb[n], r1)
        right = R.ta_apply_image(mid, r2)
        if second == 7:  # Color blends with L: the original image's gray value in place of the rotated image's
            L0 = np.repeat(R.ta_luma(rgb[n])[..., None], 3, -1)
            stale = R._ta_blend(L0, mid, r2[1:2].view(np.float32)[0])
        else:
            lut0, mean0 = R.ta_lut_mean(R.ta_histograms(R.ta_pack(rgb[n][None]))[0].numpy(), r2)
            stale = R.ta_apply_image(mid, r2, lut0, mean0)
        differs |= bool((stale != right).any())
    return differs


# ---------------------------------------------------------------------------------------------
# 6. chained samples travel
# ---------------------------------------------------------------------------------------------
TRAVEL = [(6, 5), (11, 13), (1, 9)]  # per sample: first stage, second stage (a gather, a LUT, a 3x3 op last)


@pytest.mark.parametrize("erase_mode", ["const", "pixel"])
@pytest.mark.parametrize("mix", ["paste", "blend.25", "paste+blend.25"])
@pytest.mark.parametrize("perm", PERMS)
@chain_shapes
@devices
def test_chained_samples_travel(dev, Ho, Wo, perm, mix, erase_mode):
    """A twice-augmented, erased sample travels into the paste and the blend: the float64 oracle and the bf16
    bound of test_augment_mix on the fold of the definition, exactly as for one operation."""
    rows = chain_table(TRAVEL, Ho, Wo)
    pm, w, box, noise = i32(perm, dev), 1.0, None, None
    kw = dict(perm=pm, erase=i32(ERASE, dev), erase_mode=erase_mode)
    if "paste" in mix:
        box = MIXBOX
        kw["mixbox"] = i32(MIXBOX, dev)
    if "blend" in mix:
        w = 0.25
        kw["blend"] = torch.tensor([w], dtype=F32, device=dev)
    if erase_mode == "pixel":
        kw["erase_rng"] = (SEED, i32([11], dev))
        noise = noise64(SEED, 11, N, Ho, Wo, dev)
    aug = torch.from_numpy(fold(flipped(Ho, Wo), rows)).to(dev)
    for norm in (UNIT, (MEAN, STD)):
        got = chained(dev, Ho, Wo, rows, norm, **kw)
        f, mag = (aug.double(), aug.double()) if norm is UNIT else _norm_ref(aug.double(), dev)
        ref, m = oracle(f, mag, pm, w, box, ERASE, noise)
        if norm is UNIT and w == 1.0 and erase_mode != "pixel":
            assert torch.equal(got[..., :3].double(), ref), "integers: bit for bit"
        else:
            check("chain_augment travels", dev, got[..., :3], ref, bf16_bound(ref, m), what=f"{mix} {erase_mode}")


# ---------------------------------------------------------------------------------------------
# 7. K = 1 and the all-Identity table
# ---------------------------------------------------------------------------------------------
@chain_shapes
@devices
def test_one_stage_and_identity_give_the_single_call(dev, Ho, Wo):
    img = torch.from_numpy(images(Ho, Wo, "varied")).to(dev)
    bx = torch.tensor([(0.3, 1.7, Ho - 3.1, Wo - 2.3), (0.0, 0.0, Ho, Wo), (1.1, 0.2, Ho - 2.0, Wo - 1.0)], dtype=F32,
                      device=dev)
    fl = torch.tensor(FLIPS, dtype=torch.uint8, device=dev)
    kw = dict(perm=i32([2, 0, 1], dev), mixbox=i32(MIXBOX, dev), blend=torch.tensor([0.25], dtype=F32, device=dev),
              erase=i32(ERASE, dev), erase_mode="pixel", erase_rng=(SEED, i32([5], dev)))

    def single(rows):
        out = G((N, Ho, Wo, 4), BF, dev)
        work = torch.zeros(K.ta_work_words(N, Ho, Wo), dtype=torch.int32, device=dev)
        K.trivial_augment_u8(img, out.t, bx, MEAN, STD, fl, torch.from_numpy(rows).to(dev), work, **kw)
        return out.t

    def chain(rows):
        out = G((N, Ho, Wo, 4), BF, dev)
        work = torch.full((K.ta_work_words(N, Ho, Wo, len(rows)),), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        K.chain_augment_u8(img, out.t, bx, MEAN, STD, fl, torch.from_numpy(rows).to(dev), work, **kw)
        out.check()
        return out.t

    rows = table([(5, 40.5), (13, 0.0), (8, 1.5)], Ho, Wo)
    assert K.ta_work_words(N, Ho, Wo, 1) == K.ta_work_words(N, Ho, Wo)
    assert torch.equal(chain(rows[None]), single(rows)), "K = 1: the bits of trivial_augment_u8"
    ident = np.zeros((N, 8), dtype=np.int32)
    assert torch.equal(chain(np.zeros((2, N, 8), dtype=np.int32)), single(ident)), "Identity twice: Identity once"


def test_work_buffer_layout():
    n, Ho, Wo = 3, 8, 12
    assert K.ta_work_words(n, Ho, Wo, 1) == K.ta_work_words(n, Ho, Wo) == n * Ho * Wo + n * 1217
    for k in (2, 3, 4):
        words = K.ta_work_words(n, Ho, Wo, k)
        assert words == 2 * n * Ho * Wo + k * n * 1024 + n * 193, "two T, one histogram set per stage, one lut / mean"
        work = torch.zeros(words, dtype=torch.int32)
        T, hist, lut, mean = K.ta_work_views(work, n, Ho, Wo, k)
        assert tuple(T.shape) == (2, n, Ho, Wo, 4) and tuple(hist.shape) == (k, n, 4, 256) and hist.is_contiguous()
        assert tuple(lut.shape) == (n, 3, 256) and tuple(mean.shape) == (n,)
        ends = [(t.data_ptr() - work.data_ptr(), t.numel() * t.element_size()) for t in (T, hist, lut, mean)]
        assert ends[0][0] == 0 and all(a + b == c for (a, b), (c, _) in zip(ends, ends[1:]))
        assert ends[-1][0] + ends[-1][1] == 4 * words
    one = K.ta_work_views(torch.zeros(K.ta_work_words(n, Ho, Wo), dtype=torch.int32), n, Ho, Wo)
    assert tuple(one[0].shape) == (n, Ho, Wo, 4) and tuple(one[1].shape) == (n, 4, 256)


# ---------------------------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------------------------
@devices
def test_refusals(dev):
    Ho, Wo = 16, 16
    rgb, rows = images(Ho, Wo, "varied"), table([(5, 40.5), (13, 0.0), (9, 1.99)], Ho, Wo)
    T, ops, lut, tmean = prepared(rgb, rows, dev)
    out, hist = torch.empty_like(T), torch.zeros(N, 4, 256, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="alias"):
        K.ta_stage_u8(T, T, hist, ops, lut, tmean)
    both = torch.zeros(2 * T.numel() - 4 * Wo, dtype=torch.uint8, device=dev)  # (overlapping by one row)
    with pytest.raises(ValueError, match="alias"):
        K.ta_stage_u8(both[:T.numel()].view(T.shape), both[-T.numel():].view(T.shape), hist, ops, lut, tmean)
    with pytest.raises(ValueError):
        K.ta_stage_u8(T, out[:2], hist, ops, lut, tmean)
    with pytest.raises(ValueError, match="ops"):
        K.ta_stage_u8(T, out, hist, ops[:2], lut, tmean)
    with pytest.raises(ValueError, match="hist"):
        K.ta_stage_u8(T, out, hist[:2], ops, lut, tmean)
    with pytest.raises(ValueError, match="lut"):
        K.ta_stage_u8(T, out, hist, ops, lut[:2], tmean)
    with pytest.raises(TypeError, match="ops"):
        K.ta_stage_u8(T, out, hist, ops.float(), lut, tmean)
    with pytest.raises(TypeError, match="T_out"):
        K.ta_stage_u8(T, out.int(), hist, ops, lut, tmean)
    with pytest.raises(TypeError, match="hist"):
        K.ta_stage_u8(T, out, hist.float(), ops, lut, tmean)
    if dev != "cpu":  # the kernel reads T and lut as 32-bit words
        odd = torch.zeros(lut.numel() + 4, dtype=torch.uint8, device=dev)[1:1 + lut.numel()].view(lut.shape)
        with pytest.raises(ValueError, match="aligned"):
            K.ta_stage_u8(T, out, hist, ops, odd, tmean)
    K.ta_stage_u8(T, out, hist, ops, lut, tmean)  # (and this is accepted)

    img = torch.from_numpy(rgb).to(dev)
    bx = torch.tensor([(0.0, 0.0, Ho, Wo)] * N, dtype=F32, device=dev)
    fl = torch.tensor(FLIPS, dtype=torch.uint8, device=dev)
    res = torch.empty(N, Ho, Wo, 4, dtype=BF, device=dev)
    chain = torch.zeros(2, N, 8, dtype=torch.int32, device=dev)
    work = torch.zeros(K.ta_work_words(N, Ho, Wo, 2), dtype=torch.int32, device=dev)

    def call(img=img, ops=chain, work=work, **kw):
        K.chain_augment_u8(img, res, bx, MEAN, STD, fl, ops, work, **kw)

    with pytest.raises(ValueError, match="3-channel"):
        call(img=img[..., :1].contiguous())
    for k in (0, 5):
        with pytest.raises(ValueError, match="stages"):
            call(ops=torch.zeros(k, N, 8, dtype=torch.int32, device=dev),
                 work=torch.zeros(K.ta_work_words(N, Ho, Wo, 4) * 2, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="stages"):
        K.ta_work_words(N, Ho, Wo, 5)
    for bad in (chain[0], chain[:, :2], torch.zeros(2, N, 7, dtype=torch.int32, device=dev)):
        with pytest.raises(ValueError, match="ops"):
            call(ops=bad)
    with pytest.raises(TypeError, match="ops"):
        call(ops=chain.float())
    with pytest.raises(ValueError, match="work"):
        call(work=work[:-1])
    with pytest.raises(ValueError, match="work"):
        call(work=torch.zeros(K.ta_work_words(N, Ho, Wo), dtype=torch.int32, device=dev))  # (sized for one stage)
    with pytest.raises(TypeError, match="work"):
        call(work=work.float())
    with pytest.raises(ValueError, match="perm"):
        call(blend=torch.tensor([0.5], dtype=F32, device=dev))
    call(perm=i32([2, 0, 1], dev), mixbox=i32(MIXBOX, dev), erase=i32(ERASE, dev))  # (and this is accepted)
