"""resample_u8_kernel (csrc/input_resample.hip) against the float64 definition of ops/reference.py, at the shapes
where it can go wrong. Boxes are dyadic with l / n exact in fp32, so no window edge can flip between fp32 and float64."""
import numpy as np
import pytest
import torch

from dbx_distributed_pytorch_examples_amd.data.loader import pack_images
from dbx_distributed_pytorch_examples_amd.ops import kernels as K
from dbx_distributed_pytorch_examples_amd.ops import reference as R

pytestmark = pytest.mark.gpu
FILTERS = ["aa_bilinear", "bicubic", "aa_bicubic"]
MEAN, STD, DEV = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225), "cuda:0"
# (H, W, Ho, Wo, box); the kernel's limits: 16 rows a chunk, 256 columns a pass, 16 taps in LDS, 4096 staged bytes a row
CASES = {
    "many-taps": (37, 53, 8, 8, (0, 0, 37, 53)),
    "upscale": (20, 20, 16, 16, (3.25, 2.5, 6.5, 7.75)),
    "past-two-edges": (20, 20, 8, 8, (-4, -2, 16, 16)),
    "outside": (20, 20, 8, 8, (40, 40, 8, 8)),
    "ho19-short-last-chunk": (40, 31, 19, 9, (1.5, 0.5, 38, 27)),
    "ho16-one-chunk": (40, 31, 16, 9, (1.5, 0.5, 32, 27)),
    "ho17-two-chunks": (40, 31, 17, 9, (1.5, 0.5, 34, 27)),
    "column-tiling": (5, 640, 3, 300, (0.25, 1.25, 4.5, 637.5)),
    "wo256-one-pass": (4, 300, 2, 256, (0, 2, 4, 256)),
    "wo257-two-passes": (4, 300, 2, 257, (0, 2, 4, 257)),
    "row-not-stageable": (3, 1400, 2, 100, (0, 0, 3, 1400)),
    "taps-16": (8, 128, 8, 16, (0, 0, 8, 128)),
    "taps-17": (8, 136, 8, 16, (0, 0, 8, 136)),
}


def run_t(img, boxes, flip, Ho, Wo, name, **kw):
    n = boxes.shape[0]
    T = torch.full((n, Ho, Wo, 4), 7, dtype=torch.uint8, device=DEV)
    hist = torch.zeros(n, 4, 256, dtype=torch.int32, device=DEV)
    K.crop_resize_u8(img, T, hist, boxes, flip, resample=name, **kw)
    return T, hist


def check_against_definition(T, hist, imgs, boxes, flip, name):
    """u8 differs from the definition's rounding only where v64 is within eps of the boundary, and is within 0.5 + eps
    of v64 everywhere; L and the histograms are exact. Returns (values that differ, largest (|u8 - v64| - 0.5) / eps)."""
    _, Ho, Wo, _ = T.shape
    t = T.cpu().numpy()
    worst, differ = -np.inf, 0
    for n, (v, eps) in enumerate(R.resample_v64(imgs, Ho, Wo, boxes.cpu(), flip.cpu(), name)):
        u8 = t[n, ..., :3].astype(np.float64)
        vc, eps = np.clip(v, 0.0, 255.0), eps[..., None]
        want = np.floor(vc + 0.5)
        off = u8 != want
        edge = np.abs(vc - (np.minimum(u8, want) + 0.5))
        assert (np.abs(u8 - want)[off] == 1).all() and (edge[off] <= np.broadcast_to(eps, off.shape)[off]).all()
        assert (np.abs(u8 - vc) <= 0.5 + eps).all()
        worst, differ = max(worst, float(((np.abs(u8 - vc) - 0.5) / eps).max())), differ + int(off.sum())
    assert np.array_equal(t[..., 3], R.ta_luma(t[..., :3]))
    assert torch.equal(hist.cpu(), R.ta_histograms(T).view(hist.shape))
    return differ, worst


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("name", FILTERS)
def test_t_mode_against_the_definition(name, case):
    H, W, Ho, Wo, box = CASES[case]
    img = np.random.default_rng(H * W + Ho).integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    img = torch.from_numpy(img).repeat(2, 1, 1, 1)  # the same image twice: un-flipped and flipped
    boxes, flip = torch.tensor([box, box], dtype=torch.float32), torch.tensor([0, 1], dtype=torch.uint8)
    T, hist = run_t(img.to(DEV), boxes.to(DEV), flip.to(DEV), Ho, Wo, name)
    differ, worst = check_against_definition(T, hist, img, boxes, flip, name)
    print(f"{name} {case}: {differ} values off the definition's rounding, largest (|u8 - v64| - 0.5) / eps {worst:.3f}")
    assert torch.equal(T[1], T[0].flip(1))  # the flipped sample is the mirrored one, bit for bit


@pytest.mark.parametrize("name", FILTERS)
def test_staging_limit(name):
    """Rows of 4096 bytes are staged in LDS, rows of 4112 are gathered from global memory: a ragged pair."""
    rs = np.random.default_rng(3)
    imgs = [rs.integers(0, 256, (2, w, 3), dtype=np.uint8) for w in (1365, 1366)]
    arena, table = pack_images(imgs, 3)
    assert table[:, 3].tolist() == [4096, 4112]
    boxes = torch.tensor([(0, 8, 2, 1344)] * 2, dtype=torch.float32)
    flip = torch.tensor([1, 0], dtype=torch.uint8)
    T, hist = run_t(torch.from_numpy(arena).to(DEV), boxes.to(DEV), flip.to(DEV), 2, 64, name,
                    src=torch.from_numpy(table).to(DEV))
    check_against_definition(T, hist, [torch.from_numpy(a) for a in imgs], boxes, flip, name)


@pytest.mark.parametrize("name", FILTERS)
def test_ragged_is_the_dense_call_per_sample_and_image_mode_is_the_identity_table(name):
    rs = np.random.default_rng(5)
    sizes = [(1, 1), (48, 64), (33, 47), (9, 11), (37, 64), (2, 3)]
    imgs = [rs.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    arena, table = pack_images(imgs, 3)
    table[3] = (table[3, 0], *sizes[3], 24)  # a stride that is no multiple of 16: unusable
    imgs[3] = arena[:3].reshape(1, 1, 3)  # ... and read as the arena's first pixel
    n, Ho, Wo = len(sizes), 19, 21
    boxes = torch.tensor([(0.3 * (k % 2), -0.6, 0.8 * imgs[k].shape[0] + 0.1, 1.1 * imgs[k].shape[1]) for k in range(n)],
                         dtype=torch.float32).to(DEV)
    flip = torch.from_numpy(rs.integers(0, 2, n).astype(np.uint8)).to(DEV)
    src = dict(src=torch.from_numpy(table).to(DEV))
    T, hist = run_t(torch.from_numpy(arena).to(DEV), boxes, flip, Ho, Wo, name, **src)
    for k in range(n):
        Tk, hk = run_t(torch.from_numpy(imgs[k][None].copy()).to(DEV), boxes[k:k + 1], flip[k:k + 1], Ho, Wo, name)
        assert torch.equal(T[k], Tk[0]) and torch.equal(hist[k], hk[0]), k
    out = torch.full((n, Ho, Wo, 4), float("nan"), dtype=torch.bfloat16, device=DEV)
    K.augment_u8(torch.from_numpy(arena).to(DEV), out, boxes, MEAN, STD, flip, resample=name, **src)
    want = torch.full_like(out, float("nan"))
    ops = torch.zeros(n, 8, dtype=torch.int32, device=DEV)
    lut, tmean = torch.zeros(n, 3, 256, dtype=torch.uint8, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV)
    K.ta_apply_u8(T, want, ops, lut, tmean, MEAN, STD)
    assert torch.equal(out, want)
    gray = torch.from_numpy(rs.integers(0, 256, (2, 40, 40, 1), dtype=np.uint8)).to(DEV)
    a, b = (torch.full((2, Ho, Wo, 4), float("nan"), dtype=torch.bfloat16, device=DEV) for _ in range(2))
    gb = torch.tensor([(1.5, 2.0, 38.0, 31.5)] * 2, dtype=torch.float32, device=DEV)
    K.augment_u8(gray, a, gb, MEAN, STD, flip[:2], resample=name)
    K.augment_u8(gray.expand(2, 40, 40, 3).contiguous(), b, gb, MEAN, STD, flip[:2], resample=name)
    assert torch.equal(a, b)

