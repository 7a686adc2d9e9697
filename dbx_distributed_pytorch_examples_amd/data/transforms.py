"""Image transforms (torchvision is not installed on this image).

CPU-side, torchvision-compatible semantics for the transforms the reference uses
(`utils/hf_dataset_utilities.py:58-81`, `03_composer/01_cifar_composer_resnet.ipynb:207-215`,
`02_deepspeed/03_1k_imagenet_deepspeed_resnet.py:43-53`): Compose, Resize, CenterCrop,
RandomCrop(pad), RandomResizedCrop, RandomHorizontalFlip, TrivialAugmentWide, RandAugment, AutoAugment, Grayscale,
ToTensor, Normalize, Lambda.
Inputs: PIL images or uint8 HWC numpy arrays.

For the native engine the heavy per-sample work moves to the GPU instead: the loader ships
uint8 HWC batches and ``ops.kernels.augment_u8`` does crop / bilinear resize / flip /
normalise into bf16 NHWC4 — the CPU only decodes.

Quirk NOT replicated: the reference applies train-time random augmentation
to validation data (``default_image_transforms`` for the test split); ``default_image_transforms
(train=False)`` here is deterministic.
"""
from __future__ import annotations

import math
import random
from typing import Callable, List, Sequence, Tuple, Union

import numpy as np
import torch

try:
    from PIL import Image, ImageEnhance, ImageOps
except Exception:  # pragma: no cover
    Image = ImageEnhance = ImageOps = None

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
CIFAR_MEAN = (0.4914, 0.4822, 0.4465)
CIFAR_STD = (0.2470, 0.2435, 0.2616)
MNIST_MEAN, MNIST_STD = (0.1307,), (0.3081,)


def _to_pil(img):
    if Image is not None and isinstance(img, Image.Image):
        return img
    a = np.asarray(img)
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[..., 0]
    return Image.fromarray(a)


def _size(img) -> Tuple[int, int]:  # (w, h)
    if Image is not None and isinstance(img, Image.Image):
        return img.size
    a = np.asarray(img)
    return a.shape[1], a.shape[0]


class Compose:
    def __init__(self, transforms: Sequence[Callable]):
        self.transforms = list(transforms)

    def __call__(self, x):
        for t in self.transforms:
            x = t(x)
        return x


class Lambda:
    def __init__(self, fn):
        self.fn = fn

    def __call__(self, x):
        return self.fn(x)


class Resize:
    """``Resize((h, w))`` exact, or ``Resize(s)`` = shorter side to s (bilinear)."""

    def __init__(self, size):
        self.size = size

    def __call__(self, img):
        img = _to_pil(img)
        w, h = img.size
        if isinstance(self.size, int):
            if w <= h:
                nw, nh = self.size, int(round(h * self.size / w))
            else:
                nh, nw = self.size, int(round(w * self.size / h))
        else:
            nh, nw = self.size
        return img.resize((nw, nh), Image.BILINEAR)


class CenterCrop:
    def __init__(self, size):
        self.size = (size, size) if isinstance(size, int) else tuple(size)

    def __call__(self, img):
        img = _to_pil(img)
        w, h = img.size
        th, tw = self.size
        left, top = int(round((w - tw) / 2.0)), int(round((h - th) / 2.0))
        return img.crop((left, top, left + tw, top + th))


class RandomCrop:
    def __init__(self, size, padding: int = 0):
        self.size = (size, size) if isinstance(size, int) else tuple(size)
        self.padding = padding

    def __call__(self, img):
        a = np.asarray(_to_pil(img))
        if self.padding:
            pad = [(self.padding, self.padding), (self.padding, self.padding)] + ([(0, 0)] if a.ndim == 3 else [])
            a = np.pad(a, pad)
        h, w = a.shape[:2]
        th, tw = self.size
        i, j = random.randint(0, h - th), random.randint(0, w - tw)
        return Image.fromarray(np.ascontiguousarray(a[i:i + th, j:j + tw]))


def random_resized_crop_box(w: int, h: int, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), rng=random):
    """torchvision's RandomResizedCrop box sampling: returns (top, left, height, width)."""
    area = h * w
    log_r = (math.log(ratio[0]), math.log(ratio[1]))
    for _ in range(10):
        target = area * rng.uniform(*scale)
        ar = math.exp(rng.uniform(*log_r))
        cw = int(round(math.sqrt(target * ar)))
        ch = int(round(math.sqrt(target / ar)))
        if 0 < cw <= w and 0 < ch <= h:
            return rng.randint(0, h - ch), rng.randint(0, w - cw), ch, cw
    in_ratio = w / h
    if in_ratio < ratio[0]:
        cw, ch = w, int(round(w / ratio[0]))
    elif in_ratio > ratio[1]:
        ch, cw = h, int(round(h * ratio[1]))
    else:
        cw, ch = w, h
    return (h - ch) // 2, (w - cw) // 2, ch, cw


class RandomResizedCrop:
    def __init__(self, size, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3)):
        self.size = (size, size) if isinstance(size, int) else tuple(size)
        self.scale, self.ratio = scale, ratio

    def __call__(self, img):
        img = _to_pil(img)
        w, h = img.size
        t, l, ch, cw = random_resized_crop_box(w, h, self.scale, self.ratio)
        return img.resize(self.size[::-1], Image.BILINEAR, box=(l, t, l + cw, t + ch))


class RandomHorizontalFlip:
    def __init__(self, p: float = 0.5):
        self.p = p

    def __call__(self, img):
        if random.random() < self.p:
            img = _to_pil(img)
            return img.transpose(Image.FLIP_LEFT_RIGHT)
        return img


class TrivialAugmentWide:
    """torchvision's ``TrivialAugmentWide(num_bins=31)`` on PIL images (nearest interpolation, black fill): one of
    fourteen operations per image, at one of ``num_bins`` strengths, with a random sign where the operation has
    one. It sits where torchvision puts it: after the crop and the flip, before ``ToTensor``.

    :meth:`apply` takes a row of the table the native engine's kernels take (``engine.mix.ta_row`` /
    ``sample_trivial_augment``) and performs it with Pillow's own ``ImageEnhance`` / ``ImageOps`` /
    ``Image.transform``, so it is also the oracle that ``ops/reference.py`` is tested against."""

    def __init__(self, num_bins: int = 31):
        from ..engine.mix import validate_auto_augment
        validate_auto_augment("ta_wide", num_bins)
        self.num_bins = num_bins

    def __call__(self, img):
        from ..engine.mix import TA_KINDS, ta_magnitude, ta_row
        img = _to_pil(img)
        kind, i, sign = random.randrange(TA_KINDS), random.randrange(self.num_bins), random.randrange(2)
        return self.apply(img, ta_row(kind, ta_magnitude(kind, i, sign, self.num_bins), img.size[1], img.size[0]))

    @staticmethod
    def apply(img, row):
        """``row``: int32 [8] = (kind, p, a, b, c, d, e, f), all but the kind fp32 bits."""
        img = _to_pil(img).convert("RGB")
        row = np.asarray(row, dtype=np.int32)
        kind = int(row[0])
        par = [float(v) for v in row[1:].view(np.float32)]
        p = par[0]
        if kind == 0:
            return img
        if 1 <= kind <= 5:  # (kind 5's matrix is the one Image.rotate builds: the same pixels)
            return img.transform(img.size, Image.AFFINE, tuple(par[1:7]), Image.NEAREST, fillcolor=0)
        if kind == 6:
            return ImageEnhance.Brightness(img).enhance(p)
        if kind == 7:
            return ImageEnhance.Color(img).enhance(p)
        if kind == 8:
            return ImageEnhance.Contrast(img).enhance(p)
        if kind == 9:
            return ImageEnhance.Sharpness(img).enhance(p)
        if kind == 10:
            return ImageOps.posterize(img, int(p))
        if kind == 11:
            return ImageOps.solarize(img, p)
        if kind == 12:
            return ImageOps.autocontrast(img)
        if kind == 13:
            return ImageOps.equalize(img)
        raise ValueError(f"unknown TrivialAugmentWide kind {kind}")


def _apply_chain(img, rows):
    """``rows`` int32 [K, 8]: :meth:`TrivialAugmentWide.apply` folded over the K rows, in order."""
    for row in np.asarray(rows, dtype=np.int32).reshape(-1, 8):
        img = TrivialAugmentWide.apply(img, row)
    return _to_pil(img).convert("RGB")


class RandAugment:
    """torchvision's ``RandAugment(num_ops=2, magnitude=9, num_magnitude_bins=31)`` on PIL images (nearest
    interpolation, black fill): ``num_ops`` operations in sequence, each a uniform choice of the fourteen at the
    fixed bin ``magnitude``. :meth:`apply` folds :meth:`TrivialAugmentWide.apply` over the rows of one sample of
    the native engine's chain table (``engine.mix.sample_rand_augment``): the Pillow oracle of
    ``K.chain_augment_u8``."""

    def __init__(self, num_ops: int = 2, magnitude: int = 9, num_bins: int = 31):
        from ..engine.mix import validate_auto_augment
        validate_auto_augment("ra", num_bins, num_ops, magnitude)
        self.num_ops, self.magnitude, self.num_bins = num_ops, magnitude, num_bins

    def __call__(self, img):
        from ..engine.mix import TA_KINDS, ra_table
        img = _to_pil(img)
        kind = [random.randrange(TA_KINDS) for _ in range(self.num_ops)]
        sign = [random.randrange(2) for _ in range(self.num_ops)]
        return self.apply(img, ra_table(kind, [self.magnitude] * self.num_ops, sign, img.size[1], img.size[0],
                                        self.num_bins))

    apply = staticmethod(_apply_chain)


class AutoAugment:
    """torchvision's ``AutoAugment(AutoAugmentPolicy.IMAGENET)`` on PIL images: one of 25 sub-policies per image,
    each of its two operations applied with its probability (``engine.mix.AA_IMAGENET`` / ``aa_table``; Invert is
    Solarize at threshold 0). :meth:`apply` as :class:`RandAugment`'s."""

    def __init__(self, policy: str = "imagenet"):
        if policy != "imagenet":
            raise ValueError(f'only the "imagenet" policy is built, got {policy!r}')
        self.policy = policy

    def __call__(self, img):
        from ..engine.mix import AA_IMAGENET, aa_table
        img = _to_pil(img)
        sub = [random.randrange(len(AA_IMAGENET))]
        u = [[random.random()], [random.random()]]
        sign = [[random.randrange(2)], [random.randrange(2)]]
        return self.apply(img, aa_table(sub, u, sign, img.size[1], img.size[0])[:, 0])

    apply = staticmethod(_apply_chain)


class Grayscale:
    def __init__(self, num_output_channels: int = 1):
        self.n = num_output_channels

    def __call__(self, img):
        g = _to_pil(img).convert("L")
        return g.convert("RGB") if self.n == 3 else g


class ToTensor:
    """PIL / uint8 HWC -> float CHW in [0, 1]."""

    def __call__(self, img):
        a = np.asarray(_to_pil(img) if not isinstance(img, np.ndarray) else img)
        if a.ndim == 2:
            a = a[:, :, None]
        return torch.from_numpy(np.array(a.transpose(2, 0, 1), copy=True)).float().div_(255.0)


class PILToUint8HWC:
    """Decode only: PIL -> uint8 HWC numpy (the native loader's CPU transform)."""

    def __init__(self, channels: int = 3):
        self.channels = channels

    def __call__(self, img):
        img = _to_pil(img)
        img = img.convert("RGB" if self.channels == 3 else "L")
        a = np.asarray(img)
        return a if a.ndim == 3 else a[:, :, None]


class Normalize:
    def __init__(self, mean, std):
        self.mean = torch.tensor(mean).view(-1, 1, 1)
        self.std = torch.tensor(std).view(-1, 1, 1)

    def __call__(self, t: torch.Tensor):
        return (t - self.mean) / self.std


def gray_to_rgb(x: torch.Tensor) -> torch.Tensor:
    return x.repeat(3, 1, 1) if x.size(0) == 1 else x


def default_image_transforms(image_size: int, normalize_transform: bool = True, convert_rgb: bool = True,
                             train: bool = True, grayscale_first: bool = False) -> Compose:
    """`utils/hf_dataset_utilities.py:58-81` (+ the 03a variant's leading ``Grayscale(3)``, `03a…:116`)."""
    t: List[Callable] = []
    if grayscale_first:
        t.append(Grayscale(3))
    t.append(Resize((image_size, image_size)))
    if train:
        t.append(RandomHorizontalFlip())
    t.append(ToTensor())
    if convert_rgb:
        t.append(Lambda(gray_to_rgb))
    if normalize_transform:
        t.append(Normalize(IMAGENET_MEAN, IMAGENET_STD))
    return Compose(t)


def cifar_transforms(train: bool = True) -> Compose:
    if train:
        return Compose([RandomCrop(32, padding=4), RandomHorizontalFlip(), ToTensor(), Normalize(CIFAR_MEAN, CIFAR_STD)])
    return Compose([ToTensor(), Normalize(CIFAR_MEAN, CIFAR_STD)])


def imagenet_transforms(train: bool = True, size: int = 224) -> Compose:
    if train:
        return Compose([RandomResizedCrop(size), RandomHorizontalFlip(), ToTensor(), Normalize(IMAGENET_MEAN, IMAGENET_STD)])
    return Compose([Resize(int(size * 256 / 224)), CenterCrop(size), ToTensor(), Normalize(IMAGENET_MEAN, IMAGENET_STD)])


def mnist_transforms(fashion: bool = False) -> Compose:
    m, s = ((0.5,), (0.5,)) if fashion else (MNIST_MEAN, MNIST_STD)
    return Compose([ToTensor(), Normalize(m, s)])
