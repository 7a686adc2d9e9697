"""Host-side sampling of the batch-mixing options of the native step: MixUp, the per-batch choice
between MixUp and CutMix, and random erasing (torchvision's ResNet-50 reference recipe, timm's "ResNet
strikes back"). Tiny numpy work per step; the device consumes what is sampled here through scalars
and small tables (``ResNetProgram.enable_mix``), so a replayed graph follows it.

Per step, from one ``numpy.random.Generator``, in this order:

1. with probability ``1 - mix_prob`` no mixing (one ``random()``, drawn only when ``mix_prob < 1``);
2. otherwise CutMix with probability ``mix_switch_prob`` when both alphas are > 0 (one ``random()``, drawn
   only then); with one alpha > 0, that one;
3. MixUp: ``lam ~ Beta(a, a)`` (``beta``), one batch permutation (``permutation``); the blend weight and the
   CE weight are both ``lam``, the box is empty;
   CutMix: ``lam ~ Beta(a, a)``, a box of area ``1 - lam`` at a uniform centre, clipped, ``lam`` re-derived
   from the clipped area, one permutation (``beta``, ``integers``, ``integers``, ``permutation``: with only
   ``cutmix_alpha`` set this is the whole sequence, the one the trainer has always drawn); blend weight 1;
4. the erase boxes (:func:`sample_erase_boxes`), drawn only when ``erase_prob > 0``;
5. the TrivialAugmentWide table (:func:`sample_trivial_augment`), drawn only with ``auto_augment="ta_wide"``;
   with ``"ra"`` the RandAugment chain (:func:`sample_rand_augment`) and with ``"aa_imagenet"`` AutoAugment's
   ImageNet policy (:func:`sample_auto_augment`) instead.

MixUp and CutMix are never both applied in one step.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

ERASE_MODES = ("const", "pixel")


def validate_mix(mixup_alpha=0.0, cutmix_alpha=0.0, mix_prob=1.0, mix_switch_prob=0.5, erase_prob=0.0,
                 erase_mode="const", erase_scale=(0.02, 1 / 3), erase_ratio=(0.3, 3.3)) -> None:
    """ValueError for a negative alpha, a probability outside [0, 1], an unknown mode or a bad range."""
    for nm, v in (("mixup_alpha", mixup_alpha), ("cutmix_alpha", cutmix_alpha)):
        if not (isinstance(v, (int, float)) and math.isfinite(v) and v >= 0):
            raise ValueError(f"{nm} must be a finite number >= 0, got {v!r}")
    for nm, v in (("mix_prob", mix_prob), ("mix_switch_prob", mix_switch_prob), ("erase_prob", erase_prob)):
        if not (isinstance(v, (int, float)) and 0.0 <= v <= 1.0):
            raise ValueError(f"{nm} must be a probability in [0, 1], got {v!r}")
    if erase_mode not in ERASE_MODES:
        raise ValueError(f"erase_mode must be one of {ERASE_MODES}, got {erase_mode!r}")
    for nm, v, top in (("erase_scale", erase_scale, 1.0), ("erase_ratio", erase_ratio, math.inf)):
        try:
            lo, hi = (float(x) for x in v)
        except (TypeError, ValueError):
            raise ValueError(f"{nm} must be a (low, high) pair, got {v!r}") from None
        if not (0.0 < lo <= hi <= top and math.isfinite(hi)):
            raise ValueError(f"{nm} must satisfy 0 < low <= high{' <= 1' if top == 1.0 else ''}, got {v!r}")


def sample_erase_boxes(rng: np.random.Generator, n: int, H: int, W: int, prob: float,
                       scale=(0.02, 1 / 3), ratio=(0.3, 3.3), tries: int = 10) -> np.ndarray:
    """torchvision's RandomErasing box rule for ``n`` samples at once: int32 [n, 4] (y0, y1, x0, x1), empty
    (all zero) for a sample that is not erased. With probability ``prob`` a sample makes up to ``tries``
    draws of ``area = H W U(scale)`` and a log-uniform aspect ratio, ``h = round(sqrt(area ar))``,
    ``w = round(sqrt(area / ar))``; the first draw with ``1 <= h < H`` and ``1 <= w < W`` wins, at a uniform
    position; a sample none of whose draws fits stays un-erased."""
    chosen = rng.random(n) < prob
    area = H * W * rng.uniform(scale[0], scale[1], (n, tries))
    ar = np.exp(rng.uniform(math.log(ratio[0]), math.log(ratio[1]), (n, tries)))
    h = np.rint(np.sqrt(area * ar)).astype(np.int64)
    w = np.rint(np.sqrt(area / ar)).astype(np.int64)
    fits = (h >= 1) & (h < H) & (w >= 1) & (w < W)
    first = fits.argmax(axis=1)
    rows = np.arange(n)
    h, w = h[rows, first], w[rows, first]
    ok = chosen & fits.any(axis=1)
    y0 = np.floor(rng.random(n) * (H - h + 1)).astype(np.int64)
    x0 = np.floor(rng.random(n) * (W - w + 1)).astype(np.int64)
    y0, x0 = np.minimum(y0, np.maximum(H - h, 0)), np.minimum(x0, np.maximum(W - w, 0))
    box = np.stack([y0, y0 + h, x0, x0 + w], axis=1)
    return np.where(ok[:, None], box, 0).astype(np.int32)


AUTO_AUGMENTS = ("ta_wide", "ra", "aa_imagenet")
TA_KINDS = 14  # Identity, ShearX, ShearY, TranslateX, TranslateY, Rotate, Brightness, Color, Contrast, Sharpness,
#                Posterize, Solarize, AutoContrast, Equalize (ops/reference.py, csrc/input_ops.hip)
TA_NAMES = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast",
            "Sharpness", "Posterize", "Solarize", "AutoContrast", "Equalize")
MAX_STAGES = 4      # operations in sequence per sample (K.chain_augment_u8)
RA_DEFAULTS = (2, 9)  # ra_num_ops, ra_magnitude
AA_NUM_BINS = 10    # torchvision's AutoAugment: _augmentation_space(10, ...)


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def validate_auto_augment(auto_augment=None, ta_num_bins=31, ra_num_ops=2, ra_magnitude=9) -> None:
    """ValueError for an unknown policy name, fewer than two magnitude bins, ``ra_num_ops`` outside 1..4 or
    ``ra_magnitude`` outside [0, ta_num_bins) with ``"ra"``, or an ``ra_*`` option away from its default while the
    policy is not ``"ra"`` (refused, never ignored)."""
    if auto_augment is not None and auto_augment not in AUTO_AUGMENTS:
        raise ValueError(f"auto_augment must be None or one of {AUTO_AUGMENTS}, got {auto_augment!r}")
    if not (_is_int(ta_num_bins) and ta_num_bins >= 2):
        raise ValueError(f"ta_num_bins must be an integer >= 2, got {ta_num_bins!r}")
    if auto_augment == "ra":
        if not (_is_int(ra_num_ops) and 1 <= ra_num_ops <= MAX_STAGES):
            raise ValueError(f"ra_num_ops must be an integer in 1..{MAX_STAGES}, got {ra_num_ops!r}")
        if not (_is_int(ra_magnitude) and 0 <= ra_magnitude < ta_num_bins):
            raise ValueError(f"ra_magnitude must be an integer bin in [0, ta_num_bins = {ta_num_bins}), got "
                             f"{ra_magnitude!r}")
    elif (ra_num_ops, ra_magnitude) != RA_DEFAULTS:
        raise ValueError(f"ra_num_ops / ra_magnitude need auto_augment='ra', the policy is {auto_augment!r}")


def auto_augment_stages(auto_augment=None, ra_num_ops=2) -> int:
    """Operations in sequence per sample: the stage count of the policy's table (0: no policy)."""
    return {None: 0, "ta_wide": 1, "ra": int(ra_num_ops), "aa_imagenet": 2}[auto_augment]


def ta_magnitude(kind: int, i: int, sign: int, num_bins: int = 31) -> float:
    """TrivialAugmentWide's magnitude of bin ``i`` (0 .. num_bins - 1) with ``sign`` (0: +, 1: -, used where
    the operation is signed): the shear m, the translation t in pixels, the angle in degrees, the enhance
    factor p, Posterize's bits, Solarize's threshold; 0 for the operations without one."""
    x = i / (num_bins - 1)
    sg = -1.0 if sign else 1.0
    if kind in (1, 2):
        return sg * 0.99 * x
    if kind in (3, 4):
        return sg * int(32.0 * x)
    if kind == 5:
        return sg * 135.0 * x
    if kind in (6, 7, 8, 9):
        return 1.0 + sg * 0.99 * x
    if kind == 10:
        return 8.0 - float(np.rint(i / ((num_bins - 1) / 6)))
    if kind == 11:
        return 255.0 - 255.0 * x
    return 0.0


def ta_row(kind: int, mag: float, Ho: int, Wo: int) -> np.ndarray:
    """One row of the device table, int32 [8] = (kind, p, a, b, c, d, e, f; all but kind fp32 bits), of an
    operation at magnitude ``mag`` (:func:`ta_magnitude`). Kinds 1-5 carry the inverse affine map of output
    pixel centres (Pillow's convention); the rotation matrix is Pillow's ``rotate`` about (Wo / 2, Ho / 2),
    computed in double and stored as fp32."""
    if not 0 <= kind < TA_KINDS:
        raise ValueError(f"kind must be in 0..{TA_KINDS - 1}, got {kind}")
    p, co = 0.0, (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    if kind == 1:
        co = (1.0, mag, 0.0, 0.0, 1.0, 0.0)
    elif kind == 2:
        co = (1.0, 0.0, 0.0, mag, 1.0, 0.0)
    elif kind == 3:
        co = (1.0, 0.0, -mag, 0.0, 1.0, 0.0)
    elif kind == 4:
        co = (1.0, 0.0, 0.0, 0.0, 1.0, -mag)
    elif kind == 5:
        al = -math.radians(mag % 360.0)
        C, S = round(math.cos(al), 15), round(math.sin(al), 15)
        cx, cy = Wo / 2.0, Ho / 2.0
        co = (C, S, (C * -cx + S * -cy) + cx, -S, C, (-S * -cx + C * -cy) + cy)  # (Pillow's order of sums)
    elif kind in (6, 7, 8, 9, 10, 11):
        p = mag
    r = np.zeros(8, dtype=np.int32)
    r[0] = kind
    r[1:].view(np.float32)[:] = (p,) + tuple(co)
    return r


def sample_trivial_augment(rng: np.random.Generator, n: int, Ho: int, Wo: int, num_bins: int = 31):
    """torchvision's TrivialAugmentWide for ``n`` samples: per sample one of the fourteen operations, one of
    ``num_bins`` magnitudes and a sign, all uniform -- always three vectorised draws (``integers(14, n)``,
    ``integers(num_bins, n)``, ``integers(2, n)``). Returns ``(kind int32 [n], rows int32 [n, 8])``."""
    kind = rng.integers(TA_KINDS, size=n)
    idx = rng.integers(num_bins, size=n)
    sign = rng.integers(2, size=n)
    return kind.astype(np.int32), ta_table(kind, idx, sign, Ho, Wo, num_bins)


def ta_table(kind, idx, sign, Ho: int, Wo: int, num_bins: int = 31) -> np.ndarray:
    """The rows of :func:`ta_row` at :func:`ta_magnitude` for arrays of kinds, bins and signs: int32 [n, 8]
    (vectorised: the trainer builds one per step; only the rotations take a Python loop)."""
    kind, idx, sign = (np.asarray(v, dtype=np.int64) for v in (kind, idx, sign))
    n = kind.shape[0]
    x = idx / (num_bins - 1)
    sg = np.where(sign != 0, -1.0, 1.0)
    par = np.zeros((n, 7))
    par[:, 1] = par[:, 5] = 1.0
    shear, trans = sg * 0.99 * x, sg * np.trunc(32.0 * x)
    par[:, 2] = np.where(kind == 1, shear, 0.0)
    par[:, 4] = np.where(kind == 2, shear, 0.0)
    par[:, 3] = np.where(kind == 3, -trans, 0.0)
    par[:, 6] = np.where(kind == 4, -trans, 0.0)
    p = np.where((kind >= 6) & (kind <= 9), 1.0 + sg * 0.99 * x, 0.0)
    p = np.where(kind == 10, 8.0 - np.rint(idx / ((num_bins - 1) / 6)), p)
    par[:, 0] = np.where(kind == 11, 255.0 - 255.0 * x, p)
    rows = np.zeros((n, 8), dtype=np.int32)
    rows[:, 0] = kind
    rows[:, 1:].view(np.float32)[:] = par
    for j in np.nonzero(kind == 5)[0]:
        rows[j] = ta_row(5, float(sg[j] * 135.0 * x[j]), Ho, Wo)
    return rows


# ---------------------------------------------------------------------------------------------
# RandAugment and the AutoAugment ImageNet policy: the same fourteen kinds and the same rows, several in
# sequence per sample (K.chain_augment_u8), on torchvision's other magnitude space
# ---------------------------------------------------------------------------------------------
_RA_SPACES: dict = {}


def _ra_space(num_bins: int, Ho: int, Wo: int) -> np.ndarray:
    """float64 [14, num_bins]: the unsigned magnitude of every kind and bin in torchvision's RandAugment /
    AutoAugment space, from the float32 ``torch.linspace(0, end, num_bins)`` (x_i below) as torchvision reads it,
    one Python float per entry: ShearX / ShearY x_i, end 0.3; TranslateX / TranslateY int(x_i) pixels, end
    150/331 of the width / height; Rotate x_i degrees, end 30; Brightness / Color / Contrast / Sharpness x_i, end
    0.9 (the factor is 1 +- x_i); Posterize 8 - round_half_even(i / ((num_bins - 1) / 4)) bits; Solarize the
    threshold ``linspace(255, 0, num_bins)[i]``; 0 for Identity / AutoContrast / Equalize."""
    key = (int(num_bins), int(Ho), int(Wo))
    if key not in _RA_SPACES:
        import torch

        def lin(a, b):
            return torch.linspace(a, b, num_bins).double().numpy()
        t = np.zeros((TA_KINDS, num_bins))
        t[1] = t[2] = lin(0.0, 0.3)
        t[3] = np.trunc(lin(0.0, 150.0 / 331.0 * Wo))
        t[4] = np.trunc(lin(0.0, 150.0 / 331.0 * Ho))
        t[5] = lin(0.0, 30.0)
        t[6] = t[7] = t[8] = t[9] = lin(0.0, 0.9)
        t[10] = 8.0 - np.rint(np.arange(num_bins) / ((num_bins - 1) / 4))
        t[11] = lin(255.0, 0.0)
        _RA_SPACES[key] = t
    return _RA_SPACES[key]


def ra_magnitudes(kind, idx, sign, num_bins: int, Ho: int, Wo: int) -> np.ndarray:
    """:func:`ra_magnitude` for arrays of kinds, bins and signs (float64, what :func:`ta_row` takes)."""
    kind, idx, sign = (np.asarray(v, dtype=np.int64) for v in (kind, idx, sign))
    base = _ra_space(num_bins, Ho, Wo)[kind, idx]
    sg = np.where(sign != 0, -1.0, 1.0)
    mag = np.where((kind >= 1) & (kind <= 5), sg * base, base)
    return np.where((kind >= 6) & (kind <= 9), 1.0 + sg * base, mag)


def ra_magnitude(kind: int, i: int, sign: int, num_bins: int, Ho: int, Wo: int) -> float:
    """The magnitude of bin ``i`` with ``sign`` (0: +, 1: -) in RandAugment's / AutoAugment's space
    (:func:`_ra_space`), in :func:`ta_row`'s units: the signed shear, translation in pixels and angle in
    degrees, the enhance factor 1 +- x_i, Posterize's bits, Solarize's threshold; 0 where there is none."""
    if not 0 <= kind < TA_KINDS:
        raise ValueError(f"kind must be in 0..{TA_KINDS - 1}, got {kind}")
    if not 0 <= i < num_bins:
        raise ValueError(f"bin must be in [0, {num_bins}), got {i}")
    return float(ra_magnitudes([kind], [i], [sign], num_bins, Ho, Wo)[0])


def ta_rows(kind, mag, Ho: int, Wo: int) -> np.ndarray:
    """:func:`ta_row` for arrays of kinds and magnitudes of any shape: int32 [..., 8] (vectorised; a rotation
    matrix is computed once per distinct angle)."""
    kind, mag = np.asarray(kind, dtype=np.int64), np.asarray(mag, dtype=np.float64)
    shape = kind.shape
    kind, mag = kind.reshape(-1), mag.reshape(-1)
    par = np.zeros((kind.shape[0], 7))
    par[:, 1] = par[:, 5] = 1.0
    par[:, 2] = np.where(kind == 1, mag, 0.0)
    par[:, 4] = np.where(kind == 2, mag, 0.0)
    par[:, 3] = np.where(kind == 3, -mag, 0.0)
    par[:, 6] = np.where(kind == 4, -mag, 0.0)
    par[:, 0] = np.where((kind >= 6) & (kind <= 11), mag, 0.0)
    rows = np.zeros((kind.shape[0], 8), dtype=np.int32)
    rows[:, 0] = kind
    rows[:, 1:].view(np.float32)[:] = par
    rot = kind == 5
    for m in np.unique(mag[rot]):
        rows[rot & (mag == m)] = ta_row(5, float(m), Ho, Wo)
    return rows.reshape(shape + (8,))


def ra_table(kind, idx, sign, Ho: int, Wo: int, num_bins: int = 31) -> np.ndarray:
    """The rows of :func:`ta_row` at :func:`ra_magnitude` for arrays of kinds, bins and signs: int32 [..., 8]."""
    return ta_rows(kind, ra_magnitudes(kind, idx, sign, num_bins, Ho, Wo), Ho, Wo)


def sample_rand_augment(rng: np.random.Generator, n: int, Ho: int, Wo: int, num_ops: int = 2, magnitude: int = 9,
                        num_bins: int = 31) -> np.ndarray:
    """torchvision's RandAugment for ``n`` samples: ``num_ops`` operations in sequence, each a uniform choice of
    the fourteen at the fixed bin ``magnitude``, with a uniform sign where the operation is signed. Two draws:
    ``integers(14, (K, n))``, ``integers(2, (K, n))``. Returns the stage-major table int32 [K, n, 8]."""
    kind = rng.integers(TA_KINDS, size=(num_ops, n))
    sign = rng.integers(2, size=(num_ops, n))
    return ra_table(kind, np.full_like(kind, magnitude), sign, Ho, Wo, num_bins)


# torchvision's AutoAugmentPolicy.IMAGENET: 25 sub-policies of two (operation, probability, bin); None: the
# operation has no magnitude. Invert is Solarize at threshold 0 (its LUT x < p ? x : 255 - x, with p = 0).
AA_IMAGENET = (
    (("Posterize", 0.4, 8), ("Rotate", 0.6, 9)),
    (("Solarize", 0.6, 5), ("AutoContrast", 0.6, None)),
    (("Equalize", 0.8, None), ("Equalize", 0.6, None)),
    (("Posterize", 0.6, 7), ("Posterize", 0.6, 6)),
    (("Equalize", 0.4, None), ("Solarize", 0.2, 4)),
    (("Equalize", 0.4, None), ("Rotate", 0.8, 8)),
    (("Solarize", 0.6, 3), ("Equalize", 0.6, None)),
    (("Posterize", 0.8, 5), ("Equalize", 1.0, None)),
    (("Rotate", 0.2, 3), ("Solarize", 0.6, 8)),
    (("Equalize", 0.6, None), ("Posterize", 0.4, 6)),
    (("Rotate", 0.8, 8), ("Color", 0.4, 0)),
    (("Rotate", 0.4, 9), ("Equalize", 0.6, None)),
    (("Equalize", 0.0, None), ("Equalize", 0.8, None)),
    (("Invert", 0.6, None), ("Equalize", 1.0, None)),
    (("Color", 0.6, 4), ("Contrast", 1.0, 8)),
    (("Rotate", 0.8, 8), ("Color", 1.0, 2)),
    (("Color", 0.8, 8), ("Solarize", 0.8, 7)),
    (("Sharpness", 0.4, 7), ("Invert", 0.6, None)),
    (("ShearX", 0.6, 5), ("Equalize", 1.0, None)),
    (("Color", 0.4, 0), ("Equalize", 0.6, None)),
    (("Equalize", 0.4, None), ("Solarize", 0.2, 4)),
    (("Solarize", 0.6, 5), ("AutoContrast", 0.6, None)),
    (("Invert", 0.6, None), ("Equalize", 1.0, None)),
    (("Color", 0.6, 4), ("Contrast", 1.0, 8)),
    (("Equalize", 0.8, None), ("Equalize", 0.6, None)),
)


def aa_kind(name: str) -> int:
    """The kind of a policy table's operation name (Invert: 11, Solarize -- at threshold 0)."""
    if name == "Invert":
        return 11
    if name not in TA_NAMES:
        raise ValueError(f"unknown operation {name!r}")
    return TA_NAMES.index(name)


def aa_applies(u, prob):
    """Whether a sub-policy's operation of probability ``prob`` applies at the uniform draw ``u`` in [0, 1):
    torchvision's ``u <= prob``, and never at ``prob`` 0."""
    return (np.asarray(u) <= prob) & (np.asarray(prob) > 0)


def aa_table(sub, u, sign, Ho: int, Wo: int, policy=AA_IMAGENET) -> np.ndarray:
    """The stage-major table int32 [2, n, 8] of sub-policies ``sub`` [n] with draws ``u`` [2, n] and signs
    [2, n]: stage j is the sub-policy's j-th operation where it applies (:func:`aa_applies`), else Identity. An
    operation's bin indexes :func:`ra_magnitude`'s space at ``AA_NUM_BINS`` = 10 bins; Invert carries threshold 0."""
    sub, u, sign = np.asarray(sub, dtype=np.int64), np.asarray(u, dtype=np.float64), np.asarray(sign, dtype=np.int64)
    kinds = np.array([[aa_kind(op[0]) for op in sp] for sp in policy], dtype=np.int64)
    probs = np.array([[op[1] for op in sp] for sp in policy])
    bins = np.array([[0 if op[2] is None else op[2] for op in sp] for sp in policy], dtype=np.int64)
    invert = np.array([[op[0] == "Invert" for op in sp] for sp in policy])
    kind, idx = kinds[sub].T, bins[sub].T  # [2, n]
    mag = np.where(invert[sub].T, 0.0, ra_magnitudes(kind, idx, sign, AA_NUM_BINS, Ho, Wo))
    on = aa_applies(u, probs[sub].T)
    return ta_rows(np.where(on, kind, 0), np.where(on, mag, 0.0), Ho, Wo)


def sample_auto_augment(rng: np.random.Generator, n: int, Ho: int, Wo: int) -> np.ndarray:
    """torchvision's AutoAugment with the ImageNet policy for ``n`` samples: one of the 25 sub-policies per
    sample, each of its two operations applied with its probability, a uniform sign where the operation is signed.
    Three draws: ``integers(25, n)``, ``random((2, n))``, ``integers(2, (2, n))``. Returns int32 [2, n, 8]."""
    sub = rng.integers(len(AA_IMAGENET), size=n)
    u = rng.random((2, n))
    sign = rng.integers(2, size=(2, n))
    return aa_table(sub, u, sign, Ho, Wo)


@dataclass
class MixDraw:
    """What one step uses: ``kind`` "none" | "mixup" | "cutmix"; ``lam`` the CE weight of the sample's own
    label; ``blend`` the input blend weight (1 unless MixUp); ``perm`` int32 [N]; ``box`` (y0, y1, x0, x1);
    ``erase`` int32 [N, 4] by source sample, or None when erasing is off; ``ta`` the TrivialAugmentWide
    table int32 [N, 8] by source sample (:func:`ta_row`), or None when the option is off; with ``"ra"`` /
    ``"aa_imagenet"`` the stage-major chain table int32 [K, N, 8]."""
    kind: str
    lam: float
    blend: float
    perm: np.ndarray
    box: Tuple[int, int, int, int]
    erase: Optional[np.ndarray]
    ta: Optional[np.ndarray] = None

    def __getitem__(self, name):  # (``last_mix["ta"]``)
        return getattr(self, name)


class MixSampler:
    def __init__(self, rng: np.random.Generator, N: int, H: int, W: int, *, mixup_alpha=0.0, cutmix_alpha=0.0,
                 mix_prob=1.0, mix_switch_prob=0.5, erase_prob=0.0, erase_scale=(0.02, 1 / 3),
                 erase_ratio=(0.3, 3.3), auto_augment=None, ta_num_bins=31, ra_num_ops=2, ra_magnitude=9):
        """``auto_augment``: None, ``"ta_wide"``, ``"ra"`` (RandAugment: ``ra_num_ops`` operations at bin
        ``ra_magnitude`` of ``ta_num_bins``) or ``"aa_imagenet"`` (AutoAugment's ImageNet policy: two stages on
        ten bins -- ``ta_num_bins`` is ignored for it)."""
        validate_mix(mixup_alpha, cutmix_alpha, mix_prob, mix_switch_prob, erase_prob, "const", erase_scale,
                     erase_ratio)
        validate_auto_augment(auto_augment, ta_num_bins, ra_num_ops, ra_magnitude)
        self.auto_augment, self.ta_num_bins = auto_augment, int(ta_num_bins)
        self.ra_num_ops, self.ra_magnitude = int(ra_num_ops), int(ra_magnitude)
        self.rng, self.N, self.H, self.W = rng, int(N), int(H), int(W)
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.mix_prob, self.mix_switch_prob = float(mix_prob), float(mix_switch_prob)
        self.erase_prob = float(erase_prob)
        self.erase_scale = tuple(float(v) for v in erase_scale)
        self.erase_ratio = tuple(float(v) for v in erase_ratio)

    def _kind(self) -> str:
        r = self.rng
        if self.mixup_alpha <= 0 and self.cutmix_alpha <= 0:
            return "none"
        if self.mix_prob < 1.0 and not r.random() < self.mix_prob:
            return "none"
        if self.mixup_alpha > 0 and self.cutmix_alpha > 0:
            return "cutmix" if r.random() < self.mix_switch_prob else "mixup"
        return "cutmix" if self.cutmix_alpha > 0 else "mixup"

    def sample(self) -> MixDraw:
        r, N, H, W = self.rng, self.N, self.H, self.W
        kind = self._kind()
        lam, blend, box = 1.0, 1.0, (0, 0, 0, 0)
        if kind == "mixup":
            # (the fp32 value the device scalars hold, so the blend and the CE weight are one number)
            lam = blend = float(np.float32(r.beta(self.mixup_alpha, self.mixup_alpha)))
            perm = r.permutation(N).astype("int32")
        elif kind == "cutmix":
            # lam ~ Beta(a, a); box of area (1 - lam) at a uniform centre, clipped; lam re-derived from
            # the clipped area (Composer's CutMix); one permutation of the batch
            lam = float(r.beta(self.cutmix_alpha, self.cutmix_alpha))
            cut = (1.0 - lam) ** 0.5
            ch, cw = int(H * cut), int(W * cut)
            cy, cx = int(r.integers(0, H)), int(r.integers(0, W))
            y0, y1 = min(max(cy - ch // 2, 0), H), min(max(cy + ch // 2, 0), H)
            x0, x1 = min(max(cx - cw // 2, 0), W), min(max(cx + cw // 2, 0), W)
            lam = 1.0 - (y1 - y0) * (x1 - x0) / float(H * W)
            box = (y0, y1, x0, x1)
            perm = r.permutation(N).astype("int32")
        else:
            perm = np.arange(N, dtype="int32")
        erase = None
        if self.erase_prob > 0:
            erase = sample_erase_boxes(r, N, H, W, self.erase_prob, self.erase_scale, self.erase_ratio)
        ta = None
        if self.auto_augment == "ta_wide":  # (after every earlier draw: the sequences without it are unchanged)
            ta = sample_trivial_augment(r, N, H, W, self.ta_num_bins)[1]
        elif self.auto_augment == "ra":
            ta = sample_rand_augment(r, N, H, W, self.ra_num_ops, self.ra_magnitude, self.ta_num_bins)
        elif self.auto_augment == "aa_imagenet":
            ta = sample_auto_augment(r, N, H, W)
        return MixDraw(kind, lam, blend, perm, box, erase, ta)
