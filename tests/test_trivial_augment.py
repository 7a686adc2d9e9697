"""Per-element checks of the TrivialAugmentWide input kernels (csrc/input_ops.hip): ``crop_resize_u8``,
``ta_prepare``, ``ta_apply_u8`` and the composed ``trivial_augment_u8``.

The rules are those of tests/test_nn_ops.py and tests/test_augment_mix.py, whose helpers are imported:
every test runs on the CPU (``ops/reference.py``, the dispatcher's CPU path) and on the GPU (the HIP
kernels); outputs start NaN-filled between guard sentinels.

Everything the operations compute is integer or fixed-order fp32 (AutoContrast: float64) arithmetic, so
the kernels are compared with the numpy definition (``reference.ta_apply_image`` / ``ta_lut_mean``, which
tests/test_trivial_augment_cpu.py pins to Pillow) BIT FOR BIT: normalising with mean 0 and std 1/255 makes
the bf16 output the augmented uint8 value itself (integers up to 256 are exact in bf16), so the public
output is compared with integers and no pixel is excused -- rotations at +-135 degrees included, because
the kernel and the definition share the fp32 formula. Where the output is not an integer (a MixUp blend,
ImageNet mean / std) the float64 oracle and ``bf16_bound`` of test_augment_mix apply unchanged: the
augmented value is an exact integer, so its chain is the plain kernel's normalisation and blend.
"""
import numpy as np
import pytest
import torch

from dbx_distributed_pytorch_examples_amd.engine import mix as M
from dbx_distributed_pytorch_examples_amd.ops import kernels as K
from dbx_distributed_pytorch_examples_amd.ops import reference as R
from test_augment_mix import INEXACT, PERMS, i32, noise64, oracle
from test_nn_ops import (AUG_CASES, AUG_STAGED, BF, DEVICES, F32, GPU_ONLY, MEAN, RATIOS, STD, G, _augment_ref, _norm_ref,
                         bf16_bound, check, gen)

devices = pytest.mark.parametrize("dev", DEVICES)
N = 3
SHAPES = [(16, 16), (24, 40), (32, 32)]
shapes = pytest.mark.parametrize("Ho,Wo", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
FLIPS = [0, 1, 1]
UNIT = ((0.0, 0.0, 0.0), (1 / 255, 1 / 255, 1 / 255))  # mean, std: the output is the uint8 value

# every kind at the extremes of its magnitude (and one value inside): (kind, magnitude)
OPS = ([(0, 0.0)]
       + [(k, m) for k in (1, 2) for m in (0.99, -0.99, 0.33)]
       + [(k, t) for k in (3, 4) for t in (32.0, -32.0, 7.0)]
       + [(5, a) for a in (4.5, 40.5, -100.3, 67.5, 121.5, 135.0, -135.0, 90.0)]
       + [(k, p) for k in (6, 7, 8, 9) for p in (0.01, 1.0, 1.99, 0.67)]
       + [(10, b) for b in (2.0, 8.0, 5.0)]
       + [(11, t) for t in (0.0, 255.0, 127.5)]
       + [(12, 0.0), (13, 0.0)])
OPS += [(0, 0.0)] * (-len(OPS) % N)
CHUNKS = [OPS[i:i + N] for i in range(0, len(OPS), N)]
chunks = pytest.mark.parametrize("ops", CHUNKS, ids=["+".join(f"{R.TA_NAMES[k]}{m:g}" for k, m in c) for c in CHUNKS])


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    mine = sorted(k for k in RATIOS if k.startswith("trivial_augment"))
    if mine:
        print("\n[test_trivial_augment] largest err / bound per test and device:")
        for k in mine:
            print(f"  {k}: {RATIOS[k]:.4f}")


def images(Ho, Wo, which):
    """uint8 [N, Ho, Wo, 3]: "varied" = random, narrow-range, ramp; "flat" = constant, one grey level per
    channel (AutoContrast's lo == hi and Equalize's single-bin paths), two levels."""
    rs = np.random.default_rng(Ho * 100 + Wo)
    if which == "varied":
        yy, xx = np.mgrid[0:Ho, 0:Wo]
        ramp = np.stack([(yy * 7 + xx * 3) % 256, (xx * 5) % 251, (yy * xx) % 256], -1)
        a = [rs.integers(0, 256, (Ho, Wo, 3)), rs.integers(40, 200, (Ho, Wo, 3)), ramp]
    else:
        a = [np.full((Ho, Wo, 3), 77), np.broadcast_to(np.array([10, 200, 77]), (Ho, Wo, 3)),
             np.where(rs.integers(0, 2, (Ho, Wo, 3)) > 0, 230, 20)]
    return np.stack(a).astype(np.uint8)


def table(ops, Ho, Wo):
    return np.stack([M.ta_row(k, m, Ho, Wo) for k, m in ops])


def prepared(rgb, rows, dev):
    """(T, ops, lut, tmean) on ``dev`` for given images: the LUTs and means from the numpy definition."""
    T = R.ta_pack(rgb)
    hist = R.ta_histograms(T).numpy()
    lm = [R.ta_lut_mean(hist[n], rows[n]) for n in range(len(rows))]
    lut = torch.from_numpy(np.stack([l for l, _ in lm]))
    tmean = torch.tensor([m for _, m in lm], dtype=torch.int32)
    return T.to(dev), torch.from_numpy(rows).to(dev), lut.to(dev), tmean.to(dev)


def definition(rgb, rows):
    """The augmented uint8 images by the numpy definition, one sample at a time."""
    return np.stack([R.ta_apply_image(rgb[n], rows[n]) for n in range(len(rows))])


def apply(dev, T, ops, lut, tmean, norm=UNIT, **kw):
    n, Ho, Wo, _ = T.shape
    out = G((n, Ho, Wo, 4), BF, dev)
    K.ta_apply_u8(T, out.t, ops, lut, tmean, norm[0], norm[1], **kw)
    out.check()
    assert torch.equal(out.t[..., 3], torch.zeros_like(out.t[..., 3])), "the pad channel is exactly 0 in every mode"
    return out.t


# ---------------------------------------------------------------------------------------------
# 2. ta_apply_u8 == the definition, bit for bit
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["varied", "flat"])
@chunks
@shapes
@devices
def test_every_kind_bit_for_bit(dev, Ho, Wo, ops, which):
    rgb, rows = images(Ho, Wo, which), table(ops, Ho, Wo)
    got = apply(dev, *prepared(rgb, rows, dev))
    want = torch.from_numpy(definition(rgb, rows).astype(np.int64))
    assert torch.equal(got[..., :3].cpu().double(), want.double()), [R.TA_NAMES[k] for k, _ in ops]


def test_the_cases_move_pixels():
    """The table above is not vacuous: every non-identity row changes its "varied" image somewhere (Posterize
    to 8 bits and an enhance factor of 1 are identities by definition)."""
    for Ho, Wo in SHAPES:
        rgb = images(Ho, Wo, "varied")
        for k, m in OPS:
            same = k == 0 or (k in (6, 7, 8, 9) and m == 1.0) or (k, m) == (10, 8.0)
            for n in range(N):
                changed = bool((R.ta_apply_image(rgb[n], M.ta_row(k, m, Ho, Wo)) != rgb[n]).any())
                if same:
                    assert not changed, (k, m)
            if not same:
                assert any((R.ta_apply_image(rgb[n], M.ta_row(k, m, Ho, Wo)) != rgb[n]).any() for n in range(N)), (k, m)


MIXBOX = [0, 9, 5, 16]
ERASE = [(3, 12, 2, 8), (0, 4, 4, 16), (8, 11, 0, 16)]  # straddle the CutMix box's bottom (y = 9) and left (x = 5) edges
MIXED = [(5, -135.0), (13, 0.0), (9, 1.99)]              # a gather, a LUT and a 3x3 op travel with their samples
SEED = 0x9E3779B97F4A7C15


@pytest.mark.parametrize("erase_mode", [None, "const", "pixel"])
@pytest.mark.parametrize("mix", ["none", "paste", "blend1", "blend.25", "paste+blend.25"])
@pytest.mark.parametrize("perm", PERMS)
@shapes
@devices
def test_augmented_samples_travel(dev, Ho, Wo, perm, mix, erase_mode):
    """An augmented, erased sample travels into the paste and the blend. Integer outputs (no blend weight
    other than 1) are compared exactly; the others with the float64 oracle and the bf16 bound."""
    rgb, rows = images(Ho, Wo, "varied"), table(MIXED, Ho, Wo)
    T, ops, lut, tmean = prepared(rgb, rows, dev)
    kw, pm, w, box, er, noise = {}, None, 1.0, None, None, None
    if mix != "none":
        pm = i32(perm, dev)
        kw["perm"] = pm
    if "paste" in mix:
        box = MIXBOX
        kw["mixbox"] = i32(MIXBOX, dev)
    if "blend" in mix:
        w = 0.25 if ".25" in mix else 1.0
        kw["blend"] = torch.tensor([w], dtype=F32, device=dev)
    if erase_mode is not None:
        er = ERASE
        kw.update(erase=i32(ERASE, dev), erase_mode=erase_mode)
        if erase_mode == "pixel":
            kw["erase_rng"] = (SEED, i32([11], dev))
            noise = noise64(SEED, 11, N, Ho, Wo, dev)
    aug = torch.from_numpy(definition(rgb, rows)).to(dev)
    for norm in (UNIT, (MEAN, STD)):
        got = apply(dev, T, ops, lut, tmean, norm, **kw)
        if norm is UNIT:
            f, mag = aug.double(), aug.double()
        else:
            f, mag = _norm_ref(aug.double(), dev)
        ref, m = oracle(f, mag, pm, w, box, er, noise)
        if norm is UNIT and w == 1.0 and erase_mode != "pixel":
            assert torch.equal(got[..., :3].double(), ref), "integers: bit for bit"
        else:
            check("trivial_augment travels", dev, got[..., :3], ref, bf16_bound(ref, m), what=f"{mix} {erase_mode}")


@devices
def test_row_wider_than_one_tile(dev):
    """1030 columns: ta_apply_u8 walks a row in tiles of 1024, and the paste box, the blend and the erase box
    all reach into the second tile, with a gather across rows and a LUT kind in the table. Image levels are
    multiples of 4 (Posterize keeps multiples of 8) and w = 1/4, so every blended value is an integer below 256,
    exact in bf16 and far from a rounding boundary: the kernel's unit normalisation (v * 1/(255 std), exactly v)
    and the reference's ((v / 255) / std, within 2^-22 of v) round to the same bits, whatever the order of the
    blend's roundings. The output equals ``reference.ta_apply_u8`` bit for bit -- on the CPU that is the function
    under test itself, so there only the assertions against ``definition()`` below carry weight."""
    n, Ho, Wo = 2, 3, 1030
    rs = np.random.default_rng(7)
    rgb = (4 * rs.integers(0, 64, (n, Ho, Wo, 3))).astype(np.uint8)
    rows = table([(5, 0.1), (10, 5.0)], Ho, Wo)  # Rotate by 0.1 degrees (0.9 rows at the row ends), Posterize
    T, ops, lut, tmean = prepared(rgb, rows, "cpu")
    kw = dict(perm=[1, 0], mixbox=[0, 2, 1000, 1030], blend=[0.25], erase=[(1, 3, 1020, 1028), (0, 0, 0, 0)])
    tens = lambda d: dict(perm=i32(kw["perm"], d), mixbox=i32(kw["mixbox"], d), erase=i32(kw["erase"], d),  # noqa: E731
                          blend=torch.tensor(kw["blend"], dtype=F32, device=d), erase_mode="const")
    want = torch.full((n, Ho, Wo, 4), float("nan"), dtype=BF)
    R.ta_apply_u8(T, want, ops, lut, tmean, *UNIT, **tens("cpu"))
    got = apply(dev, T.to(dev), ops.to(dev), lut.to(dev), tmean.to(dev), **tens(dev))
    assert torch.equal(got.cpu(), want)
    # (not vacuous: the second tile holds pasted, blended and erased pixels)
    aug = torch.from_numpy(definition(rgb, rows)).double()
    assert bool((aug[0, :, 1024:] != torch.from_numpy(rgb)[0, :, 1024:]).any()) and bool(aug[0, :, 1024:].any())
    assert torch.equal(want[1, 0, 1024:, :3].double(), aug[0, 0, 1024:])       # pasted from sample 0
    assert torch.equal(want[1, 1, 1020:1028, :3].double(), torch.zeros(8, 3))  # ... with its erase box
    assert torch.equal(want[0, 2, 1024:1028, :3], (0.75 * aug[1, 2, 1024:1028]).to(BF))  # erased, then blended
    assert torch.equal(want[0, 2, 1028:, :3], (0.25 * aug[0, 2, 1028:] + 0.75 * aug[1, 2, 1028:]).to(BF))


# ---------------------------------------------------------------------------------------------
# 3. ta_prepare
# ---------------------------------------------------------------------------------------------
def hist_images():
    rs = np.random.default_rng(3)
    lv = np.stack([rs.permutation(256) for _ in range(3)], -1).reshape(16, 16, 3)  # all 256 levels, once each
    two32 = np.where(rs.integers(0, 2, (32, 32, 3)) > 0, 201, 17)
    two16 = np.where(rs.integers(0, 2, (16, 16, 3)) > 0, 255, 0)
    return [("random", rs.integers(0, 256, (24, 40, 3))), ("narrow", rs.integers(90, 131, (32, 32, 3))),
            ("constant", np.full((16, 16, 3), 77)), ("per-channel", np.broadcast_to(np.array([0, 255, 9]), (16, 16, 3))),
            ("two-level-32", two32), ("two-level-16", two16), ("all-256", lv)]


@pytest.mark.parametrize("name,img", hist_images(), ids=[n for n, _ in hist_images()])
@devices
def test_ta_prepare(dev, name, img):
    """lut / mean equal the definition exactly, for every kind (the table has one row per kind and
    magnitude case, each with the same image's histograms)."""
    rows = np.stack([M.ta_row(k, m, 16, 16) for k, m in OPS])
    n = len(rows)
    T = R.ta_pack(img.astype(np.uint8)[None])
    hist = R.ta_histograms(T).repeat(n, 1, 1)
    lut, tmean = G((n, 3, 256), torch.uint8, dev), torch.full((n,), -7, dtype=torch.int32, device=dev)
    K.ta_prepare(hist.to(dev), torch.from_numpy(rows).to(dev), lut.t, tmean)
    lut.check()
    for j in range(n):
        l, m = R.ta_lut_mean(hist[j].numpy(), rows[j])
        assert np.array_equal(lut.t[j].cpu().numpy(), l), (name, OPS[j])
        assert int(tmean[j]) == m == (2 * int(R.ta_luma(img).sum()) + img.shape[0] * img.shape[1]) // (
            2 * img.shape[0] * img.shape[1])
        if OPS[j][0] < 10:
            assert np.array_equal(l, np.tile(np.arange(256, dtype=np.uint8), (3, 1))), "identity unless the kind is 10-13"


# ---------------------------------------------------------------------------------------------
# 4. crop_resize_u8
# ---------------------------------------------------------------------------------------------
C3_CASES = [c for c in AUG_CASES if c.values[1] == 3] + [AUG_STAGED]


def crop(dev, img, bx, fl, Ho, Wo):
    n = img.shape[0]
    T = G((n, Ho, Wo, 4), torch.uint8, dev)
    hist = torch.zeros(n, 4, 256, dtype=torch.int32, device=dev)
    K.crop_resize_u8(img, T.t, hist, bx, fl)
    T.check()
    return T.t, hist


def crop_ref(img, bx, fl, Ho, Wo):
    """float64: (v, T) with T = floor(v + 1/2) and Pillow's L in the fourth channel."""
    v = _augment_ref(img, bx, fl, Ho, Wo).cpu()
    u = torch.floor(v + 0.5).clamp(0, 255).to(torch.uint8)
    return v, R.ta_pack(u)


@pytest.mark.parametrize("Ho,Wo", [(8, 8), (16, 16), (32, 32)])  # (box sizes are Ho x a power of two at these)
@pytest.mark.parametrize("Win,Cin,Hin,boxes", C3_CASES)
@devices
def test_crop_resize_exact_boxes(dev, Win, Cin, Hin, boxes, Ho, Wo):
    """Source coordinates and weights exact in fp32: T and the histograms equal the float64 definition."""
    g = gen(dev, 20)
    img = torch.randint(0, 256, (N, Hin, Win, Cin), generator=g, device=dev, dtype=torch.uint8)
    bx = torch.tensor(boxes, dtype=F32, device=dev)
    fl = torch.tensor(FLIPS, dtype=torch.uint8, device=dev)
    T, hist = crop(dev, img, bx, fl, Ho, Wo)
    _, want = crop_ref(img, bx, fl, Ho, Wo)
    assert torch.equal(T.cpu(), want)
    assert torch.equal(hist.cpu(), R.ta_histograms(want))
    assert bool((hist.sum(-1) == Ho * Wo).all()), "every channel's histogram counts every pixel once"
    T2, hist2 = crop(dev, img, bx, None, Ho, Wo)  # (no flip table: nobody flipped)
    assert torch.equal(T2[0], T[0]) and torch.equal(T2[1], T[1].flip(1)) and torch.equal(hist2, hist)


@shapes
@devices
def test_crop_resize_inexact_boxes(dev, Ho, Wo):
    """|T - ref| <= 1 everywhere, and equal wherever the float64 value is at least 2^-10 from a half-integer
    (fp32 evaluates v to about 2^-16 of 255); the excluded share is <= 1 %, asserted on the reference first."""
    g = gen(dev, 21)
    img = torch.randint(0, 256, (N, 9, 32, 3), generator=g, device=dev, dtype=torch.uint8)
    bx = torch.tensor(INEXACT, dtype=F32, device=dev)
    fl = torch.tensor(FLIPS, dtype=torch.uint8, device=dev)
    v, want = crop_ref(img, bx, fl, Ho, Wo)
    near = ((v + 0.5) - torch.floor(v + 0.5) < 2.0 ** -10) | (torch.ceil(v + 0.5) - (v + 0.5) < 2.0 ** -10)
    share = float(near.double().mean())
    print(f"trivial_augment crop_resize inexact[{dev}] {Ho}x{Wo}: excluded share {share:.5f}")
    assert share <= 0.01
    T, hist = crop(dev, img, bx, fl, Ho, Wo)
    d = (T[..., :3].cpu().int() - want[..., :3].int()).abs()
    assert int(d.max()) <= 1
    assert int(d[~near].max()) == 0
    assert torch.equal(T.cpu()[..., 3], R.ta_pack(T[..., :3].cpu())[..., 3]), "L is Pillow's gray value of the stored pixel"
    assert torch.equal(hist.cpu(), R.ta_histograms(T.cpu())) and bool((hist.sum(-1) == Ho * Wo).all())


@pytest.mark.parametrize("dev", GPU_ONLY)
def test_grid_stride(dev):
    """4100 samples x 8 rows = 32800 rows in 4100 row chunks, more than the 4096-block grids of crop_resize_u8
    and ta_apply_u8: the composed call against the definition."""
    n, Hin, Win, Ho, Wo = 4100, 4, 16, 8, 8
    rs = np.random.default_rng(5)
    g = gen(dev, 22)
    img = torch.randint(0, 256, (n, Hin, Win, 3), generator=g, device=dev, dtype=torch.uint8)
    bx = torch.tensor([(0.0, 0.0, 4.0, 16.0), (-0.5, 2.25, 2.0, 8.0)] * (n // 2), dtype=F32, device=dev)
    fl = torch.from_numpy(rs.integers(0, 2, n).astype(np.uint8)).to(dev)
    rows = M.sample_trivial_augment(rs, n, Ho, Wo)[1]
    work = torch.zeros(K.ta_work_words(n, Ho, Wo), dtype=torch.int32, device=dev)
    out = G((n, Ho, Wo, 4), BF, dev)
    K.trivial_augment_u8(img, out.t, bx, *UNIT, fl, torch.from_numpy(rows).to(dev), work)
    out.check()
    _, want = crop_ref(img, bx, fl, Ho, Wo)
    T, hist, _, _ = K.ta_work_views(work, n, Ho, Wo)
    assert torch.equal(T.cpu(), want) and torch.equal(hist.cpu(), R.ta_histograms(want))
    aug = definition(want[..., :3].numpy(), rows)
    assert torch.equal(out.t[..., :3].cpu().double(), torch.from_numpy(aug.astype(np.float64)))


# ---------------------------------------------------------------------------------------------
# the composed call, and 5. identity
# ---------------------------------------------------------------------------------------------
def source(dev, Ho, Wo, boxes):
    g = gen(dev, 23)
    img = torch.randint(0, 256, (N, Ho + 8, Wo + 8, 3), generator=g, device=dev, dtype=torch.uint8)
    return img, torch.tensor(boxes, dtype=F32, device=dev), torch.tensor(FLIPS, dtype=torch.uint8, device=dev)


def composed(dev, img, bx, fl, Ho, Wo, rows, norm=(MEAN, STD), **kw):
    out = G((N, Ho, Wo, 4), BF, dev)
    work = torch.full((K.ta_work_words(N, Ho, Wo) + 3,), 0x5A5A5A5A, dtype=torch.int32, device=dev)  # (stale contents)
    K.trivial_augment_u8(img, out.t, bx, norm[0], norm[1], fl, torch.from_numpy(rows).to(dev), work, **kw)
    out.check()
    assert int(work[-1]) == 0x5A5A5A5A and int(work[-3]) == 0x5A5A5A5A, "nothing past ta_work_words is written"
    return out.t


@chunks
@shapes
@devices
def test_composed_call(dev, Ho, Wo, ops):
    """crop_resize_u8 -> ta_prepare -> ta_apply_u8 through one call, integer crop boxes: the definition
    applied to the cropped, flipped image, exactly."""
    boxes = [(3.0, 5.0, Ho, Wo), (0.0, 0.0, Ho, Wo), (8.0, 8.0, Ho, Wo)]
    img, bx, fl = source(dev, Ho, Wo, boxes)
    rows = table(ops, Ho, Wo)
    got = composed(dev, img, bx, fl, Ho, Wo, rows, UNIT)
    crop_ = torch.stack([img[n, int(b[0]):int(b[0]) + Ho, int(b[1]):int(b[1]) + Wo] for n, b in enumerate(boxes)]).cpu()
    crop_ = torch.stack([c.flip(1) if f else c for c, f in zip(crop_, FLIPS)]).numpy()
    assert torch.equal(got[..., :3].cpu().double(), torch.from_numpy(definition(crop_, rows).astype(np.float64)))


def plain(dev, img, bx, fl, Ho, Wo, **kw):
    out = G((N, Ho, Wo, 4), BF, dev)
    K.augment_u8(img, out.t, bx, MEAN, STD, flip=fl, **kw)
    return out.t


@pytest.mark.parametrize("form", ["plain", "mixing"])
@shapes
@devices
def test_identity_table_integer_boxes(dev, Ho, Wo, form):
    """An all-Identity table with integer, unscaled crop boxes (h = Ho, w = Wo, integer origin: CIFAR's padded
    random crop, reaching past the image) gives the bits of the call without the option."""
    boxes = [(-4.0, -4.0, Ho, Wo), (0.0, 3.0, Ho, Wo), (12.0, 12.0, Ho, Wo)]
    img, bx, fl = source(dev, Ho, Wo, boxes)
    rows = np.zeros((N, 8), dtype=np.int32)
    kw = {}
    if form == "mixing":
        kw = dict(perm=i32([2, 0, 1], dev), mixbox=i32(MIXBOX, dev), blend=torch.tensor([0.25], dtype=F32, device=dev),
                  erase=i32(ERASE, dev), erase_mode="pixel", erase_rng=(SEED, i32([5], dev)))
    assert torch.equal(composed(dev, img, bx, fl, Ho, Wo, rows, **kw), plain(dev, img, bx, fl, Ho, Wo, **kw))


@shapes
@devices
def test_identity_table_scaled_boxes(dev, Ho, Wo):
    """With scaled boxes the Identity differs from the plain call by the uint8 rounding only. Against the
    float64 un-rounded oracle: the stored value is within d = 0.5 / (255 std) of it (plus v's fp32 chain),
    and bf16 rounds the shifted value, so |got - ref| <= d + 2^-8 (|ref| + d) + 2^-20 mag."""
    g = gen(dev, 24)
    img = torch.randint(0, 256, (N, 9, 32, 3), generator=g, device=dev, dtype=torch.uint8)
    bx = torch.tensor(INEXACT, dtype=F32, device=dev)
    fl = torch.tensor(FLIPS, dtype=torch.uint8, device=dev)
    got = composed(dev, img, bx, fl, Ho, Wo, np.zeros((N, 8), dtype=np.int32))
    ref, mag = _norm_ref(_augment_ref(img, bx, fl, Ho, Wo), dev)
    d = 0.5 / (255.0 * torch.tensor(STD, dtype=torch.float64, device=dev))
    check("trivial_augment identity scaled", dev, got[..., :3], ref, d + 2.0 ** -8 * (ref.abs() + d) + 2.0 ** -20 * mag)


# ---------------------------------------------------------------------------------------------
# 8. wrapper refusals
# ---------------------------------------------------------------------------------------------
@devices
def test_refusals(dev):
    Ho, Wo = 16, 16
    img, bx, fl = source(dev, Ho, Wo, [(0.0, 0.0, Ho, Wo)] * N)
    out = torch.empty(N, Ho, Wo, 4, dtype=BF, device=dev)
    rows = torch.zeros(N, 8, dtype=torch.int32, device=dev)
    work = torch.zeros(K.ta_work_words(N, Ho, Wo), dtype=torch.int32, device=dev)

    def call(img=img, ops=rows, work=work, **kw):
        K.trivial_augment_u8(img, out, bx, MEAN, STD, fl, ops, work, **kw)

    with pytest.raises(ValueError, match="3-channel"):
        call(img=img[..., :1].contiguous())
    with pytest.raises(ValueError, match="ops"):
        call(ops=rows[:2])
    with pytest.raises(ValueError, match="ops"):
        call(ops=torch.zeros(N, 7, dtype=torch.int32, device=dev))
    with pytest.raises(TypeError, match="ops"):
        call(ops=rows.float())
    with pytest.raises(ValueError, match="work"):
        call(work=work[:-1])
    with pytest.raises(TypeError, match="work"):
        call(work=work.float())
    with pytest.raises(ValueError, match="perm"):
        call(blend=torch.tensor([0.5], dtype=F32, device=dev))
    with pytest.raises(ValueError, match="erase_rng"):
        call(erase=i32(ERASE, dev), erase_mode="pixel")
    T, hist, lut, tmean = K.ta_work_views(work, N, Ho, Wo)
    with pytest.raises(ValueError, match="3-channel"):
        K.crop_resize_u8(img[..., :1].contiguous(), T, hist, bx, fl)
    with pytest.raises(ValueError):
        K.ta_prepare(hist, rows[:2], lut, tmean)
    with pytest.raises(ValueError):
        K.ta_apply_u8(T, out, rows[:2], lut, tmean, MEAN, STD)
    call(perm=i32([2, 0, 1], dev), mixbox=i32(MIXBOX, dev), erase=i32(ERASE, dev))  # (and this is accepted)
