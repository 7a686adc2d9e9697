"""Host -> device input pipeline for the native engine.

Replaces the reference's ``DataLoader(dataset, batch_size, shuffle=True)`` with ``num_workers=0``
and per-sample PIL transforms in the training process (SURVEY.md §3 hot loop item 2, K20, K21):

1. **batch assembly on the host** into a *pinned* uint8 NHWC staging buffer — by the C++ MDS
   reader (``_C.MDSReader.gather``: memcpy of raw pixels, thread pool, GIL released) for MDS
   shards, or by a thread pool over any map-style dataset yielding fixed-size uint8 HWC images;
2. **one async H2D copy per batch** (uint8: 4x fewer PCIe bytes than the reference's fp32 tensors)
   on a dedicated copy stream, double/triple buffered so the copy of batch k+1 overlaps step k;
3. **augmentation on the GPU** inside the captured step: per-sample crop boxes + flips are sampled
   on the host (tiny) and ``augment_u8`` does RandomResizedCrop / RandomCrop(pad) / flip /
   normalise -> bf16 NHWC4 (the native program's stem input).

Ragged batches (``ragged_max_hw``): images keep their own sizes. A batch is one byte arena and a table
(``pack_layout``); only the used prefix crosses PCIe, and ``augment_u8(..., src=table)`` crops every sample from
its own geometry, so ``RandomResizedCrop`` draws scale and ratio on the original image as torchvision does.

Ranks read disjoint sample sets (``ShardSampler`` semantics; MDS: ``StreamingDataset.epoch_indices``).
Sized for 288 GB HBM: ``device_cache=True`` keeps a whole uint8 dataset resident on the GPU
(ImageNet-1K at 224x224 is ~193 GB raw, CIFAR/TinyImageNet are trivial) and skips PCIe entirely.
"""
from __future__ import annotations

import math
import random
import threading
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import Iterator, Optional, Sequence, Tuple

import numpy as np
import torch

from .transforms import random_resized_crop_box


@dataclass
class AugmentSpec:
    """What the GPU augmentation does per sample (train) — eval uses full-image / center boxes."""
    mode: str = "none"              # none | random_resized_crop | random_crop | center_crop | resize_center_crop
    scale: Tuple[float, float] = (0.08, 1.0)
    ratio: Tuple[float, float] = (3 / 4, 4 / 3)
    pad: int = 0                    # random_crop padding (CIFAR: 4)
    crop_frac: float = 0.875        # center_crop: 224/256; resize_center_crop: the side over the shorter side
    hflip: bool = False


def ceil16(x: int) -> int:
    return (int(x) + 15) & ~15


def pack_layout(hs, ws, C: int) -> Tuple[np.ndarray, int]:
    """THE layout of a ragged batch (csrc/input_ops.hip src_img and csrc/runtime/mds_loader.cpp mirror it): sample
    n of size ``hs[n] x ws[n]`` with ``C`` channels has ``stride_n = ceil16(ws[n] C)`` bytes per row and starts at
    the running sum of ``hs[k] stride_k`` over the samples before it -- a multiple of 16, so every row is 16-byte
    aligned. Returns ``(table, used)``: int32 ``[N, 4]`` = (offset / 16, H, W, stride) and the bytes of the
    arena the batch fills. The ``stride - W C`` padding bytes of a row are never read as pixels."""
    hs, ws = np.asarray(hs, dtype=np.int64).reshape(-1), np.asarray(ws, dtype=np.int64).reshape(-1)
    if hs.shape != ws.shape or (hs < 1).any() or (ws < 1).any() or C < 1:
        raise ValueError("pack_layout: one positive height and width per sample")
    stride = (ws * C + 15) // 16 * 16
    size = hs * stride
    off = np.concatenate([[0], np.cumsum(size)[:-1]]) if len(hs) else np.zeros(0, np.int64)
    used = int(size.sum())
    if used // 16 >= 2 ** 31 or (stride >= 2 ** 31).any():
        raise ValueError(f"pack_layout: a batch of {used} bytes does not fit the int32 table")
    return np.stack([off // 16, hs, ws, stride], 1).astype(np.int32).reshape(-1, 4), used


def ragged_capacity(n: int, max_hw: Tuple[int, int], C: int) -> int:
    """Bytes of an arena that holds any ``n`` images of at most ``max_hw``."""
    return int(n) * int(max_hw[0]) * ceil16(int(max_hw[1]) * C)


def pack_images(images: Sequence[np.ndarray], C: int, out: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
    """uint8 ``[H, W, C]`` images of any sizes -> ``(arena, table)`` by :func:`pack_layout`. ``out``: a 1-D uint8
    buffer to fill (its used prefix is returned); padding bytes of a fresh arena are 0."""
    table, used = pack_layout([a.shape[0] for a in images], [a.shape[1] for a in images], C)
    if out is None:
        out = np.zeros(max(used, 16), np.uint8)
    if out.ndim != 1 or out.dtype != np.uint8 or out.size < used:
        raise ValueError(f"pack_images: the batch needs {used} bytes, the buffer holds {out.size}")
    for a, (off, h, w, rb) in zip(images, table.tolist()):
        out[16 * off:16 * off + h * rb].reshape(h, rb)[:, :w * C] = np.asarray(a, np.uint8).reshape(h, w * C)
    return out[:max(used, 16)], table


def sample_boxes(n: int, hin, win, hout: int, wout: int, spec: AugmentSpec, rng: random.Random
                 ) -> Tuple[np.ndarray, np.ndarray]:
    """Per-sample crop boxes (top, left, height, width) + horizontal flips for ``augment_u8``,
    vectorised with numpy (a per-sample Python loop costs ~2-4 ms per 512-batch: a loader bottleneck
    at TinyImageNet rates). ``rng`` seeds the batch's numpy generator (reproducible per loader).
    ``hin`` / ``win``: the source size, one int for the batch or an int array ``[n]`` of per-sample sizes (a ragged
    batch: boxes are in each sample's own coordinates); constant arrays draw what the ints draw, bit for bit."""
    g = np.random.default_rng(rng.getrandbits(63))
    boxes = np.zeros((n, 4), np.float32)
    per_sample = np.ndim(hin) > 0 or np.ndim(win) > 0
    H = np.broadcast_to(np.asarray(hin, dtype=np.int64), (n,))
    W = np.broadcast_to(np.asarray(win, dtype=np.int64), (n,))
    if spec.mode == "random_resized_crop":
        # torchvision's rule: up to 10 tries of (scale, log-ratio), first fitting box wins, else centre
        area = (H * W)[:, None]
        tries = 10
        target = area * g.uniform(spec.scale[0], spec.scale[1], (n, tries))
        ar = np.exp(g.uniform(math.log(spec.ratio[0]), math.log(spec.ratio[1]), (n, tries)))
        cw = np.rint(np.sqrt(target * ar)).astype(np.int64)
        ch = np.rint(np.sqrt(target / ar)).astype(np.int64)
        ok = (cw > 0) & (cw <= W[:, None]) & (ch > 0) & (ch <= H[:, None])
        first = np.where(ok.any(1), ok.argmax(1), -1)
        rows = np.arange(n)
        h = np.where(first >= 0, ch[rows, np.maximum(first, 0)], 0)
        w = np.where(first >= 0, cw[rows, np.maximum(first, 0)], 0)
        top = (g.random(n) * (H - h + 1)).astype(np.int64)
        left = (g.random(n) * (W - w + 1)).astype(np.int64)
        # fallback (no try fit): centre crop clamped to the ratio range
        in_ratio = W / H
        narrow, wide = in_ratio < spec.ratio[0], in_ratio > spec.ratio[1]
        fh = np.where(narrow, np.rint(W / spec.ratio[0]).astype(np.int64), H)
        fw = np.where(wide & ~narrow, np.rint(H * spec.ratio[1]).astype(np.int64), W)
        miss = first < 0
        h[miss], w[miss] = fh[miss], fw[miss]
        top[miss], left[miss] = ((H - fh) // 2)[miss], ((W - fw) // 2)[miss]
        boxes[:] = np.stack([top, left, h, w], 1)
    elif spec.mode == "random_crop":
        # crop hout x wout from the image zero-padded by `pad` (pad pixels clamp to the edge here)
        if per_sample:
            boxes[:, 0] = g.integers(-spec.pad, H + spec.pad - hout + 1, n)
            boxes[:, 1] = g.integers(-spec.pad, W + spec.pad - wout + 1, n)
        else:
            boxes[:, 0] = g.integers(-spec.pad, hin + spec.pad - hout + 1, n)
            boxes[:, 1] = g.integers(-spec.pad, win + spec.pad - wout + 1, n)
        boxes[:, 2], boxes[:, 3] = hout, wout
    elif spec.mode == "center_crop":
        h, w = np.rint(H * spec.crop_frac).astype(np.int64), np.rint(W * spec.crop_frac).astype(np.int64)
        boxes[:] = np.stack([(H - h) // 2, (W - w) // 2, h, w], 1)
    elif spec.mode == "resize_center_crop":
        # torchvision's Resize(shorter side) + CenterCrop: the centred square of crop_frac times the shorter side
        side = np.rint(spec.crop_frac * np.minimum(H, W)).astype(np.int64)
        boxes[:] = np.stack([(H - side) // 2, (W - side) // 2, side, side], 1)
    else:
        boxes[:] = np.stack([np.zeros(n, np.int64), np.zeros(n, np.int64), H, W], 1)
    flips = (g.random(n) < 0.5).astype(np.uint8) if spec.hflip else np.zeros(n, np.uint8)
    return boxes, flips


OVERSIZE = ("error", "crop")


def centre_cut(a: np.ndarray, max_hw: Tuple[int, int]) -> np.ndarray:
    """``a`` [H, W, C] cut to at most ``max_hw`` around its centre (``oversize="crop"``)."""
    h, w = a.shape[:2]
    ch, cw = min(h, max_hw[0]), min(w, max_hw[1])
    y0, x0 = (h - ch) // 2, (w - cw) // 2
    return a[y0:y0 + ch, x0:x0 + cw]


class NativeImageLoader:
    """Iterates (img_u8 [B,H,W,C] device, labels [B] int64 device, boxes [B,4], flips [B]) per step.

    ``ragged_max_hw = (max_h, max_w)``: the samples keep their own sizes (``image_hw`` is unread). Iterates
    ``(packed, labels, boxes, flips, table)``: ``packed`` the 1-D uint8 bytes of the batch laid out by
    :func:`pack_layout` (only this used prefix of the worst-case pinned slot is copied to the device), ``table``
    int32 [B, 4], ``boxes`` in each sample's own coordinates. A sample above the limit raises a ValueError that
    names it (``oversize="error"``) or is cut to the limit around its centre (``"crop"``)."""

    def __init__(self, source, batch_size: int, image_hw: Tuple[int, int], device: torch.device,
                 channels: int = 3, indices_fn=None, augment: Optional[AugmentSpec] = None,
                 out_hw: Optional[Tuple[int, int]] = None, drop_last: bool = True, nthreads: int = 8,
                 prefetch: int = 2, seed: int = 0, device_cache: bool = False,
                 ragged_max_hw: Optional[Tuple[int, int]] = None, oversize: str = "error"):
        if oversize not in OVERSIZE:
            raise ValueError(f"oversize must be one of {OVERSIZE}, got {oversize!r}")
        if ragged_max_hw is None and oversize != "error":
            raise ValueError("oversize belongs to a ragged loader (ragged_max_hw=(max_h, max_w))")
        if ragged_max_hw is not None:
            if len(tuple(ragged_max_hw)) != 2 or min(int(v) for v in ragged_max_hw) < 1:
                raise ValueError(f"ragged_max_hw is (max_h, max_w), both at least 1, got {ragged_max_hw!r}")
            if device_cache:
                raise ValueError("device_cache keeps one dense uint8 tensor: it does not hold a ragged dataset")
            if out_hw is None:
                raise ValueError("a ragged loader needs out_hw: its samples have no common size")
        self.ragged = tuple(int(v) for v in ragged_max_hw) if ragged_max_hw is not None else None
        self.oversize = oversize
        self.src = source
        self.B = batch_size
        self.H, self.W = image_hw
        self.C = channels
        self.out_hw = out_hw or image_hw
        self.dev = device
        self.aug = augment or AugmentSpec()
        self.drop_last = drop_last
        self.nthreads = nthreads
        self.prefetch = max(1, prefetch)
        self.rng = random.Random(seed)
        self.indices_fn = indices_fn
        self.epoch = 0
        self.native = None
        if hasattr(source, "native_reader"):
            try:
                self.native = source.native_reader()
            except Exception:
                self.native = None  # no extension (CPU host): python gather
        pin = device.type == "cuda"
        if self.ragged is not None:  # worst-case slots; a batch fills a prefix of one
            cap = ragged_capacity(self.B, self.ragged, self.C)
            self.host = [torch.zeros(cap, dtype=torch.uint8, pin_memory=pin) for _ in range(self.prefetch + 1)]
            self.host_tab = [torch.zeros(self.B, 4, dtype=torch.int32, pin_memory=pin) for _ in range(self.prefetch + 1)]
            self.used = [0] * (self.prefetch + 1)
        else:
            self.host = [torch.empty(self.B, self.H, self.W, self.C, dtype=torch.uint8, pin_memory=pin)
                         for _ in range(self.prefetch + 1)]
        self.host_lab = [torch.empty(self.B, dtype=torch.int64, pin_memory=pin) for _ in range(self.prefetch + 1)]
        self.copy_stream = torch.cuda.Stream(device=device) if device.type == "cuda" else None
        if self.ragged is not None and self.native is not None and not hasattr(self.native, "gather_ragged"):
            self.native = None
        self.pool = ThreadPoolExecutor(max_workers=nthreads) if self.native is None else None
        self.cache = None
        if device_cache:
            self._build_device_cache()

    # ------------------------------------------------------------------------------------
    def set_epoch(self, epoch: int):
        self.epoch = epoch
        if hasattr(self.src, "set_epoch"):
            self.src.set_epoch(epoch)

    def _epoch_indices(self) -> np.ndarray:
        if self.indices_fn is not None:
            return np.asarray(self.indices_fn(self.epoch), dtype=np.int64)
        if hasattr(self.src, "epoch_indices"):
            return np.asarray(self.src.epoch_indices(), dtype=np.int64)
        return np.arange(len(self.src), dtype=np.int64)

    def __len__(self) -> int:
        n = len(self._epoch_indices())
        return n // self.B if self.drop_last else math.ceil(n / self.B)

    def _item(self, i: int):
        it = self.src[int(i)]
        if isinstance(it, dict):
            img, y = it["image"], it["label"]
        else:
            img, y = it
        a = np.asarray(img, dtype=np.uint8)
        if a.ndim == 2:
            a = a[:, :, None]
        if self.ragged is not None:
            if a.ndim != 3 or a.shape[2] != self.C or min(a.shape[:2]) < 1:
                raise ValueError(f"sample {i}: shape {a.shape}, loader expects [H, W, {self.C}]")
            if a.shape[0] > self.ragged[0] or a.shape[1] > self.ragged[1]:
                if self.oversize == "error":
                    raise ValueError(f"sample {i}: {a.shape[0]} x {a.shape[1]} exceeds ragged_max_hw={self.ragged} "
                                     '(raise the limit, write the dataset with shorter_side=, or oversize="crop")')
                a = centre_cut(a, self.ragged)
            return a, int(y)
        if a.shape != (self.H, self.W, self.C):
            raise ValueError(f"sample {i}: shape {a.shape}, loader expects {(self.H, self.W, self.C)} "
                             "(resize on the writer side or use a Resize transform)")
        return a, int(y)

    def _fill_ragged(self, slot: int, ids: np.ndarray):
        buf, lab, tab = self.host[slot], self.host_lab[slot], self.host_tab[slot]
        n = len(ids)
        if self.native is not None:
            self.used[slot] = int(self.native.gather_ragged(
                np.ascontiguousarray(ids), buf.data_ptr(), buf.numel(), tab.data_ptr(), lab.data_ptr(), self.ragged[0],
                self.ragged[1], self.C, self.oversize == "crop", "image", "label", self.nthreads))
            return
        items = list(self.pool.map(lambda k: self._item(ids[k]), range(n)))  # decoded in the pool
        table, used = pack_layout([a.shape[0] for a, _ in items], [a.shape[1] for a, _ in items], self.C)
        nb, lb = buf.numpy(), lab.numpy()
        tab.numpy()[:n] = table
        rows = table.tolist()

        def one(k):
            (a, y), (off, h, w, rb) = items[k], rows[k]
            nb[16 * off:16 * off + h * rb].reshape(h, rb)[:, :w * self.C] = a.reshape(h, w * self.C)
            lb[k] = y
        list(self.pool.map(one, range(n)))
        self.used[slot] = used

    def _fill(self, slot: int, ids: np.ndarray):
        if self.ragged is not None:
            return self._fill_ragged(slot, ids)
        buf, lab = self.host[slot], self.host_lab[slot]
        if self.native is not None:
            self.native.gather(np.ascontiguousarray(ids), buf.data_ptr(), lab.data_ptr(), self.H, self.W, self.C,
                               "image", "label", self.nthreads)
            return
        nb = buf.numpy()
        lb = lab.numpy()

        def one(k):
            a, y = self._item(ids[k])
            nb[k] = a
            lb[k] = y
        list(self.pool.map(one, range(len(ids))))

    def _build_device_cache(self):
        ids = np.arange(len(self.src) if not hasattr(self.src, "num_samples") else self.src.num_samples)
        imgs = torch.empty(len(ids), self.H, self.W, self.C, dtype=torch.uint8, device=self.dev)
        labs = torch.empty(len(ids), dtype=torch.int64, device=self.dev)
        for s in range(0, len(ids), self.B):
            chunk = ids[s:s + self.B]
            self._fill(0, chunk)
            imgs[s:s + len(chunk)].copy_(self.host[0][:len(chunk)])
            labs[s:s + len(chunk)].copy_(self.host_lab[0][:len(chunk)])
        self.cache = (imgs, labs)

    def __iter__(self) -> Iterator:
        ids = self._epoch_indices()
        nb = len(ids) // self.B if self.drop_last else math.ceil(len(ids) / self.B)
        Ho, Wo = self.out_hw
        if self.cache is not None:
            imgs, labs = self.cache
            for b in range(nb):
                sel = torch.from_numpy(ids[b * self.B:(b + 1) * self.B]).to(self.dev)
                boxes, flips = sample_boxes(len(sel), self.H, self.W, Ho, Wo, self.aug, self.rng)
                yield (imgs.index_select(0, sel), labs.index_select(0, sel),
                       torch.from_numpy(boxes).to(self.dev), torch.from_numpy(flips).to(self.dev))
            return
        # host assembly runs ahead in a background thread (bounded by the staging ring)
        ring = len(self.host)
        ready = [threading.Event() for _ in range(nb)]
        errs = []

        def producer():
            try:
                for b in range(nb):
                    if b >= ring:
                        consumed[b - ring].wait()
                    self._fill(b % ring, ids[b * self.B:(b + 1) * self.B])
                    ready[b].set()
            except BaseException as e:  # noqa: BLE001
                errs.append(e)
                for ev in ready:
                    ev.set()

        consumed = [threading.Event() for _ in range(nb)]
        th = threading.Thread(target=producer, daemon=True)
        th.start()
        try:
            for b in range(nb):
                ready[b].wait()
                if errs:
                    raise errs[0]
                slot = b % ring
                n = min(self.B, len(ids) - b * self.B)
                tab = None
                if self.ragged is not None:  # the used prefix of the slot; boxes from each sample's own size
                    take, tab = max(self.used[slot], 16), self.host_tab[slot][:n]
                    hw = tab.numpy()
                    boxes, flips = sample_boxes(n, hw[:, 1].astype(np.int64), hw[:, 2].astype(np.int64), Ho, Wo,
                                                self.aug, self.rng)
                else:
                    take = n
                    boxes, flips = sample_boxes(n, self.H, self.W, Ho, Wo, self.aug, self.rng)
                if self.copy_stream is not None:
                    with torch.cuda.stream(self.copy_stream):
                        img = self.host[slot][:take].to(self.dev, non_blocking=True)
                        tab = tab.to(self.dev, non_blocking=True) if tab is not None else None
                        lab = self.host_lab[slot][:n].to(self.dev, non_blocking=True)
                        bx = torch.from_numpy(boxes).to(self.dev, non_blocking=True)
                        fl = torch.from_numpy(flips).to(self.dev, non_blocking=True)
                        ev = torch.cuda.Event()
                        ev.record(self.copy_stream)
                    torch.cuda.current_stream(self.dev).wait_event(ev)
                    for t in (img, lab, bx, fl) + ((tab,) if tab is not None else ()):
                        t.record_stream(torch.cuda.current_stream(self.dev))
                    # the pinned slot may be refilled once this copy has executed
                    ev.synchronize() if b + ring >= nb else None
                    consumed[b].set() if b + ring >= nb else _set_after(ev, consumed[b])
                else:
                    img = self.host[slot][:take].clone()
                    tab = tab.clone() if tab is not None else None
                    lab = self.host_lab[slot][:n].clone()
                    bx, fl = torch.from_numpy(boxes), torch.from_numpy(flips)
                    consumed[b].set()
                if tab is not None:
                    yield img, lab, bx, fl, tab
                else:
                    yield img, lab, bx, fl
        finally:
            for ev in consumed:
                ev.set()
            th.join(timeout=30)


def _set_after(cuda_event, flag: threading.Event):
    """Set ``flag`` once ``cuda_event`` completes, without blocking the training thread."""
    def waiter():
        cuda_event.synchronize()
        flag.set()
    threading.Thread(target=waiter, daemon=True).start()
