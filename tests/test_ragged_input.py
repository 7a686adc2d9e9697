"""Ragged sources of the input kernels (csrc/input_ops.hip, the RAGGED instantiations of augment_u8,
augment_mix_u8 and crop_resize_u8): a batch of uint8 images of different sizes as one byte arena and a table
int32 [N, 4] = (offset / 16, H, W, stride) (data/loader.py ``pack_layout``).

Every test runs on the CPU (``ops/reference.py``, the definition) and on the GPU (the HIP kernels), with the
helpers and rules of tests/test_nn_ops.py. All criteria but one are exact: a ragged call is compared bit for bit
with the dense call on the same pixels, which every other input test already pins. The one bound, the MixUp
blend of two sources of different sizes, is ``bf16_bound`` against the float64 per-sample oracle with
test_augment_mix's magnitude rule ``mag = w mag_n + (1 - w) mag_p``; its boxes are exact in fp32.

Fixture: five sources of (H, W) = (1, 1), (3, 5), (8, 16), (7, 11), (2, 1400) with 1 and 3 channels -- a stride
equal to the row (16 x 3 bytes), padded strides, and (3 channels) a 4200-byte row that cannot be staged in LDS
-- outputs 8 x 8 and 5 x 7, boxes whose source coordinates are not exact in fp32 and reach past the image, flips.
"""
import numpy as np
import pytest
import torch

from dbx_distributed_pytorch_examples_amd.data.loader import pack_images, pack_layout
from dbx_distributed_pytorch_examples_amd.engine.mix import ta_rows
from dbx_distributed_pytorch_examples_amd.ops import kernels as K
from dbx_distributed_pytorch_examples_amd.ops import reference as R
from test_nn_ops import BF, DEVICES, F32, GPU_ONLY, MEAN, RATIOS, STD, G, _augment_ref, _norm_ref, bf16_bound, check

devices = pytest.mark.parametrize("dev", DEVICES)
SHAPES = [(1, 1), (3, 5), (8, 16), (7, 11), (2, 1400)]
FLIPS = [0, 1, 1, 0, 1]
OUTS = [(8, 8), (5, 7)]
outs = pytest.mark.parametrize("Ho,Wo", OUTS)
chans = pytest.mark.parametrize("Cin", [1, 3])
SEED = 0x9E3779B97F4A7C15
SENTINEL = 0xA5


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    for k in sorted(k for k in RATIOS if k.startswith("ragged")):
        print(f"  {k}: {RATIOS[k]:.4f}")


def i32(x, dev):
    return torch.tensor(x, dtype=torch.int32, device=dev)


def images(shapes, C, seed=31):
    rs = np.random.default_rng(seed)
    return [rs.integers(0, 256, (h, w, C), dtype=np.uint8) for h, w in shapes]


def inexact_boxes(shapes):
    """(y0, x0, h, w) in each sample's own coordinates: not exact in fp32, partly outside the image."""
    return [(-0.3 + 0.1 * n, 0.2 - 0.37 * n, 0.9 * h + 0.7, 0.77 * w + 1.3) for n, (h, w) in enumerate(shapes)]


def packed(imgs, C, dev):
    """(arena, table) on ``dev``; the arena starts 16-byte aligned (torch allocations are) so rows can be staged."""
    arena, table = pack_images(imgs, C)
    return torch.from_numpy(arena.copy()).to(dev), torch.from_numpy(table).to(dev)


def aug(dev, img, bx, fl, Ho, Wo, n=None, **kw):
    n = img.shape[0] if n is None else n
    out = G((n, Ho, Wo, 4), BF, dev)
    K.augment_u8(img, out.t, bx, MEAN, STD, flip=fl, **kw)
    out.check()
    assert torch.equal(out.t[..., 3], torch.zeros_like(out.t[..., 3])), "the pad channel is exactly 0"
    assert torch.isfinite(out.t.float()).all(), "every element written"
    return out.t


def crop(dev, img, bx, fl, Ho, Wo, n, **kw):
    T = G((n, Ho, Wo, 4), torch.uint8, dev)
    hist = torch.zeros(n, 4, 256, dtype=torch.int32, device=dev)
    K.crop_resize_u8(img, T.t, hist, bx, fl, **kw)
    T.check()
    return T.t, hist


def fixture(dev, Cin, shapes=SHAPES, flips=FLIPS, boxes=None):
    imgs = images(shapes, Cin)
    arena, table = packed(imgs, Cin, dev)
    bx = torch.tensor(boxes or inexact_boxes(shapes), dtype=F32, device=dev)
    fl = torch.tensor(flips, dtype=torch.uint8, device=dev)
    return imgs, arena, table, bx, fl


# ---------------------------------------------------------------------------------------------
# (a) a ragged row is the dense call on that sample alone
# ---------------------------------------------------------------------------------------------
@outs
@chans
@devices
def test_ragged_row_equals_the_dense_call_on_that_sample(dev, Cin, Ho, Wo):
    imgs, arena, table, bx, fl = fixture(dev, Cin)
    assert table[:, 3].tolist() == [16, 16, 16 * Cin, 16 if Cin == 1 else 48, 1408 if Cin == 1 else 4208]
    got = aug(dev, arena, bx, fl, Ho, Wo, n=len(imgs), src=table, src_channels=Cin)
    for n, a in enumerate(imgs):
        one = torch.from_numpy(a[None]).to(dev)
        want = aug(dev, one, bx[n:n + 1], fl[n:n + 1], Ho, Wo)
        assert torch.equal(got[n], want[0]), f"sample {n} {a.shape}"


@outs
@devices
def test_ragged_crop_resize_equals_the_dense_call_on_that_sample(dev, Ho, Wo):
    imgs, arena, table, bx, fl = fixture(dev, 3)
    T, hist = crop(dev, arena, bx, fl, Ho, Wo, len(imgs), src=table)
    for n, a in enumerate(imgs):
        one = torch.from_numpy(a[None]).to(dev)
        Tn, hn = crop(dev, one, bx[n:n + 1], fl[n:n + 1], Ho, Wo, 1)
        assert torch.equal(T[n], Tn[0]) and torch.equal(hist[n], hn[0]), f"sample {n} {a.shape}"
    assert hist.sum().item() == len(imgs) * 4 * Ho * Wo


# ---------------------------------------------------------------------------------------------
# (b) a ragged batch of equal sizes is the dense batch, under every option
# ---------------------------------------------------------------------------------------------
# 33-byte rows (dense: gathered from global memory; ragged: staged with a 48-byte stride) and 96-byte rows (both
# staged)
@pytest.mark.parametrize("Hin,Win", [(9, 11), (9, 32)])
@devices
def test_equal_sizes_equal_the_dense_call(dev, Hin, Win):
    n, Ho, Wo = 3, 8, 8
    shapes = [(Hin, Win)] * n
    imgs, arena, table, bx, fl = fixture(dev, 3, shapes, [0, 1, 1])
    dense = torch.from_numpy(np.stack(imgs)).to(dev)
    pm, box = i32([0, 2, 1], dev), i32([0, 5, 3, Wo], dev)  # (sample 0 is the permutation's fixed point)
    er = i32([(3, 7, 1, 5), (0, 0, 0, 0), (4, 6, 0, 8)], dev)
    rng = (SEED, i32([11], dev))
    w03, w1 = torch.tensor([0.3], dtype=F32, device=dev), torch.ones(1, dtype=F32, device=dev)
    options = [dict(), dict(perm=pm, mixbox=box), dict(perm=pm, blend=w03), dict(perm=pm, blend=w1),
               dict(perm=pm, mixbox=box, blend=w03), dict(erase=er), dict(erase=er, erase_mode="pixel", erase_rng=rng),
               dict(perm=pm, mixbox=box, blend=w03, erase=er, erase_mode="pixel", erase_rng=rng)]
    for kw in options:
        want = aug(dev, dense, bx, fl, Ho, Wo, **kw)
        got = aug(dev, arena, bx, fl, Ho, Wo, n=n, src=table, **kw)
        assert torch.equal(got, want), sorted(kw)
    # TrivialAugment and a chain of two operations (a gather, a LUT from the histograms, a 3x3 operation)
    one = torch.from_numpy(ta_rows([5, 13, 9], [40.5, 0.0, 1.99], Ho, Wo)).to(dev)
    two = torch.from_numpy(np.stack([ta_rows([6, 11, 1], [0.67, 127.5, 0.33], Ho, Wo),
                                     ta_rows([5, 13, 9], [40.5, 0.0, 1.99], Ho, Wo)])).to(dev)
    mixkw = dict(perm=pm, mixbox=box, blend=w03, erase=er, erase_mode="pixel", erase_rng=rng)
    for fn, ops, stages in ((K.trivial_augment_u8, one, 1), (K.chain_augment_u8, two, 2)):
        for kw in (dict(), mixkw):
            res = []
            for img, skw in ((dense, {}), (arena, dict(src=table, src_channels=3))):
                out = G((n, Ho, Wo, 4), BF, dev)
                work = torch.zeros(K.ta_work_words(n, Ho, Wo, stages), dtype=torch.int32, device=dev)
                fn(img, out.t, bx, MEAN, STD, fl, ops, work, **kw, **skw)
                out.check()
                res.append(out.t)
            assert torch.equal(res[0], res[1]), (fn.__name__, sorted(kw))


# ---------------------------------------------------------------------------------------------
# (c) a CutMix paste over sources of different sizes: the composition of the two plain ragged outputs
# ---------------------------------------------------------------------------------------------
@outs
@chans
@devices
def test_cutmix_over_different_sizes(dev, Cin, Ho, Wo):
    imgs, arena, table, bx, fl = fixture(dev, Cin)
    n = len(imgs)
    perm = [4, 1, 0, 2, 3]  # (sample 1 is a fixed point; the unstageable source is pasted into the 1 x 1 one)
    y0, y1, x0, x1 = 1, Ho - 2, 2, Wo
    plain = aug(dev, arena, bx, fl, Ho, Wo, n=n, src=table, src_channels=Cin)
    want = plain.clone()
    want[:, y0:y1, x0:x1] = plain[torch.tensor(perm, device=dev)][:, y0:y1, x0:x1]
    kw = dict(perm=i32(perm, dev), mixbox=i32([y0, y1, x0, x1], dev), src=table, src_channels=Cin)
    assert torch.equal(aug(dev, arena, bx, fl, Ho, Wo, n=n, **kw), want), "the plain kernel"
    got = aug(dev, arena, bx, fl, Ho, Wo, n=n, blend=torch.ones(1, dtype=F32, device=dev), **kw)
    assert torch.equal(got, want), "the mixing kernel (w == 1)"
    assert not torch.equal(want, plain)


# ---------------------------------------------------------------------------------------------
# (d) a blend over different sizes against the float64 per-sample oracle
# ---------------------------------------------------------------------------------------------
def exact_boxes(shapes, Ho, Wo):
    """Sizes Ho (Wo) times a power of two and origins on multiples of 1/4: every source coordinate and weight is
    exact in fp32 (test_nn_ops AUG_CASES), some boxes reaching past the image."""
    return [(-1.25 + 0.5 * n, 0.75 - 0.25 * n, Ho * (1, 0.5, 1, 2, 0.25)[n % 5], Wo * (0.25, 0.5, 2, 1, 128)[n % 5])
            for n in range(len(shapes))]


@outs
@chans
@devices
def test_blend_over_different_sizes(dev, Cin, Ho, Wo):
    boxes = exact_boxes(SHAPES, Ho, Wo)
    imgs, arena, table, bx, fl = fixture(dev, Cin, boxes=boxes)
    n = len(imgs)
    perm = [4, 1, 0, 2, 3]
    v = torch.cat([_augment_ref(torch.from_numpy(a[None]).to(dev), bx[k:k + 1], fl[k:k + 1], Ho, Wo)
                   for k, a in enumerate(imgs)])
    f, mag = _norm_ref(v, dev)
    pl = torch.tensor(perm, device=dev)
    for w in (0.3, 0.0):
        w32 = float(torch.tensor(w, dtype=F32).double())
        ref, m = w32 * f + (1.0 - w32) * f[pl], w32 * mag + (1.0 - w32) * mag[pl]
        got = aug(dev, arena, bx, fl, Ho, Wo, n=n, perm=i32(perm, dev), blend=torch.tensor([w], dtype=F32, device=dev),
                  src=table, src_channels=Cin)
        check("ragged blend", dev, got[..., :3], ref, bf16_bound(ref, m), what=f"C{Cin} {Ho}x{Wo} w={w}")


# ---------------------------------------------------------------------------------------------
# (e) the guard: an unusable table row reads as (0, 1, 1, 16) and is never dereferenced
# ---------------------------------------------------------------------------------------------
@chans
@devices
def test_unusable_rows_read_as_the_substitute(dev, Cin):
    Ho, Wo = 8, 8
    imgs = images([(3, 5), (4, 7)], Cin)
    arena_np, table_np = pack_images(imgs, Cin)
    used = arena_np.size
    assert used % 16 == 0
    margin = 4096  # sentinel bytes on each side: an absent guard would still read only this allocation
    buf = torch.full((used + 2 * margin,), SENTINEL, dtype=torch.uint8, device=dev)
    arena = buf[margin:margin + used]
    arena.copy_(torch.from_numpy(arena_np.copy()))
    a16 = used // 16
    good = table_np[1].tolist()
    bad = [[a16 - 1, 4, 7, 32 if Cin == 3 else 16],      # starts inside, ends past the arena (by < margin)
           [a16, 1, 1, 16],                               # starts at the end
           [0, a16 + 1, 1, 16],                           # one row too many
           [good[0], 0, 7, good[3]],                      # H = 0
           [good[0], 4, 0, good[3]],                      # W = 0
           [0, 1, 7, 16 if Cin == 3 else 0],              # stride < W C
           [0, 2, 2, 24],                                 # stride % 16 != 0
           [-1, 1, 1, 16]]                                # a negative offset
    n = len(bad) + 1
    table = i32(bad + [good], dev)
    assert R.ragged_rows(table.cpu(), a16, Cin) == [R.RAGGED_SUBSTITUTE] * len(bad) + [tuple(good)]
    bx = torch.tensor([(-0.3, 0.2, 3.1, 5.3)] * n, dtype=F32, device=dev)
    fl = torch.tensor([k & 1 for k in range(n)], dtype=torch.uint8, device=dev)
    sub = i32([list(R.RAGGED_SUBSTITUTE)] * len(bad) + [good], dev)
    pm = i32(list(range(1, n)) + [0], dev)
    for kw in (dict(), dict(perm=pm, blend=torch.tensor([0.3], dtype=F32, device=dev))):
        got = aug(dev, arena, bx, fl, Ho, Wo, n=n, src=table, src_channels=Cin, **kw)
        want = aug(dev, arena, bx, fl, Ho, Wo, n=n, src=sub, src_channels=Cin, **kw)
        assert torch.equal(got, want), sorted(kw)
    if Cin == 3:
        T, hist = crop(dev, arena, bx, fl, Ho, Wo, n, src=table)
        Tw, hw = crop(dev, arena, bx, fl, Ho, Wo, n, src=sub)
        assert torch.equal(T, Tw) and torch.equal(hist, hw)
        # the substitute is the arena's first pixel, everywhere
        px = arena[:3].tolist()
        assert T[0, ..., :3].reshape(-1, 3).unique(dim=0).tolist() == [px]
    assert bool((buf[:margin] == SENTINEL).all()) and bool((buf[margin + used:] == SENTINEL).all())


# ---------------------------------------------------------------------------------------------
# (f) more rows than the grid has blocks
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", GPU_ONLY)
def test_grid_stride(dev):
    """130 samples x 32 rows = 4160 rows, more than the 4096-block grid; four tiny shapes cycling; paste, blend and
    erase on. The CPU definition is bit-equal to the kernels at these boxes only by (a), so the reference here is
    the dense GPU call per shape."""
    n, Ho, Wo = 130, 32, 32
    cyc = [(1, 1), (3, 5), (4, 16), (2, 7)]
    shapes = [cyc[k % 4] for k in range(n)]
    rs = np.random.default_rng(7)
    imgs, arena, table, bx, fl = fixture(dev, 3, shapes, rs.integers(0, 2, n).tolist())
    got = aug(dev, arena, bx, fl, Ho, Wo, n=n, src=table)
    for c, (h, w) in enumerate(cyc):
        idx = list(range(c, n, 4))
        dense = torch.from_numpy(np.stack([imgs[k] for k in idx])).to(dev)
        want = aug(dev, dense, bx[idx], fl[idx], Ho, Wo)
        assert torch.equal(got[idx], want), (h, w)
    # the mixing form over the whole grid: the composition of the plain outputs where it is exact (paste, w == 1)
    perm = rs.permutation(n).tolist()
    box = [3, 20, 5, 31]
    mixed = aug(dev, arena, bx, fl, Ho, Wo, n=n, src=table, perm=i32(perm, dev), mixbox=i32(box, dev),
                blend=torch.ones(1, dtype=F32, device=dev), erase=i32([(0, 0, 0, 0)] * n, dev))
    want = got.clone()
    want[:, 3:20, 5:31] = got[torch.tensor(perm, device=dev)][:, 3:20, 5:31]
    assert torch.equal(mixed, want)
    T, hist = crop(dev, arena, bx, fl, Ho, Wo, n, src=table)
    assert hist.view(n, 4, 256).sum(2).eq(Ho * Wo).all()


# ---------------------------------------------------------------------------------------------
# (g) refusals, before any launch
# ---------------------------------------------------------------------------------------------
@devices
def test_refusals(dev):
    Ho, Wo = 8, 8
    imgs, arena, table, bx, fl = fixture(dev, 3)
    n = len(imgs)
    out = torch.empty(n, Ho, Wo, 4, dtype=BF, device=dev)

    def call(img=arena, src=table, **kw):
        K.augment_u8(img, out, bx, MEAN, STD, flip=fl, src=src, **kw)

    call()
    with pytest.raises(TypeError):
        call(src=table.long())
    with pytest.raises(ValueError):
        call(src=table[:4])
    with pytest.raises(ValueError):
        call(src=table.view(-1))
    with pytest.raises(ValueError):
        call(src=torch.zeros(n, 3, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        call(img=arena.view(1, -1))
    with pytest.raises(TypeError):
        call(img=arena.to(torch.int8))
    with pytest.raises(ValueError):
        call(img=arena[:15])
    for c in (0, 2, 4, True, 3.0):
        with pytest.raises(ValueError):
            call(src_channels=c)
    ops = torch.from_numpy(ta_rows([0] * n, [0.0] * n, Ho, Wo)).to(dev)
    work = torch.zeros(K.ta_work_words(n, Ho, Wo, 2), dtype=torch.int32, device=dev)
    T, hist = torch.empty(n, Ho, Wo, 4, dtype=torch.uint8, device=dev), torch.zeros(n, 4, 256, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="src_channels"):
        K.crop_resize_u8(arena, T, hist, bx, fl, src=table, src_channels=1)
    with pytest.raises(ValueError, match="src_channels"):
        K.trivial_augment_u8(arena, out, bx, MEAN, STD, fl, ops, work, src=table, src_channels=1)
    with pytest.raises(ValueError, match="src_channels"):
        K.chain_augment_u8(arena, out, bx, MEAN, STD, fl, ops[None], work, src=table, src_channels=1)
    with pytest.raises(TypeError):
        K.normalize_u8(arena, out, MEAN, STD, src=table)
    with pytest.raises(TypeError):
        K.augment_u8(arena, out, bx, MEAN, STD, fl, None, None, table)  # keyword-only


def test_pack_layout_is_the_tables_definition():
    table, used = pack_layout([h for h, _ in SHAPES], [w for _, w in SHAPES], 3)
    assert table.dtype == np.int32 and table.shape == (5, 4)
    assert table.tolist() == [[0, 1, 1, 16], [1, 3, 5, 16], [4, 8, 16, 48], [28, 7, 11, 48], [49, 2, 1400, 4208]]
    assert used == 16 * 49 + 2 * 4208
    views = R.ragged_views(torch.from_numpy(pack_images(images(SHAPES, 3), 3)[0].copy()), torch.from_numpy(table), 3)
    assert all(np.array_equal(v.numpy(), a) for v, a in zip(views, images(SHAPES, 3)))
