"""The host side of ragged input batches: ``pack_layout`` (the one layout definition), the loader's Python path and
the C++ reader's ``gather_ragged`` (same bytes, same table), the oversize rules, a short last batch, per-sample
``sample_boxes``, the ``resize_center_crop`` mode, the config options, and ``train()`` on an ImageFolder of PNGs
of several sizes."""
import math
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image

from dbx_distributed_pytorch_examples_amd import config as C
from dbx_distributed_pytorch_examples_amd.data.loader import (AugmentSpec, NativeImageLoader, pack_images, pack_layout,
                                                              ragged_capacity, sample_boxes)
from dbx_distributed_pytorch_examples_amd.ops import _ext
from dbx_distributed_pytorch_examples_amd.ops import reference as R

CPU = torch.device("cpu")
SIZES = [(40, 52), (33, 47), (64, 36), (48, 48), (37, 70), (1, 1), (9, 11)]


def dataset(n, C_=3, sizes=SIZES, seed=0):
    rs = np.random.default_rng(seed)
    return [(rs.integers(0, 256, sizes[i % len(sizes)] + (C_,), dtype=np.uint8), i % 5) for i in range(n)]


def pixels(packed, table, C_):
    """The pixel bytes of a batch, sample by sample (padding left out)."""
    return [v.numpy().copy() for v in R.ragged_views(packed, table, C_)]


# ---------------------------------------------------------------------------------------------
def test_pack_layout():
    hs, ws = [1, 3, 8, 7, 2], [1, 5, 16, 11, 1400]
    for C_ in (1, 3):
        table, used = pack_layout(hs, ws, C_)
        assert table.dtype == np.int32 and table.shape == (5, 4)
        off = 0
        for (o16, h, w, rb), H, W in zip(table.tolist(), hs, ws):
            assert (h, w) == (H, W) and rb == (W * C_ + 15) // 16 * 16 and rb % 16 == 0 and rb - W * C_ < 16
            assert o16 * 16 == off
            off += H * rb
        assert used == off
    assert pack_layout([4], [16], 3)[0].tolist() == [[0, 4, 16, 48]]  # a stride equal to the row
    assert pack_layout([], [], 3)[1] == 0
    for bad in (([0], [4]), ([4], [0]), ([4, 4], [4])):
        with pytest.raises(ValueError):
            pack_layout(*bad, 3)
    assert ragged_capacity(8, (48, 64), 3) == 8 * 48 * 192 and ragged_capacity(2, (5, 5), 1) == 2 * 5 * 16
    imgs = [a for a, _ in dataset(7)]
    arena, table = pack_images(imgs, 3)
    assert arena.size == pack_layout([a.shape[0] for a in imgs], [a.shape[1] for a in imgs], 3)[1]
    got = pixels(torch.from_numpy(arena.copy()), torch.from_numpy(table), 3)
    assert all(np.array_equal(g, a) for g, a in zip(got, imgs))


@pytest.mark.parametrize("C_", [1, 3])
def test_python_path_on_a_list_dataset(C_):
    ds = dataset(10, C_)
    if C_ == 1:
        ds = [(a[..., 0], y) for a, y in ds]  # (2-D gray images gain their channel axis)
    ld = NativeImageLoader(ds, 4, (0, 0), CPU, channels=C_, out_hw=(32, 32), drop_last=False, nthreads=3,
                           ragged_max_hw=(64, 72), augment=AugmentSpec(mode="random_resized_crop", hflip=True))
    assert len(ld) == 3
    seen = 0
    for packed, lab, boxes, flips, table in ld:
        n = lab.shape[0]
        assert n == (4 if seen < 8 else 2), "a short last batch"
        want = [np.asarray(a).reshape(a.shape[0], a.shape[1], C_) for a, _ in ds[seen:seen + n]]
        wt, used = pack_layout([a.shape[0] for a in want], [a.shape[1] for a in want], C_)
        assert packed.dtype == torch.uint8 and packed.dim() == 1 and packed.numel() == used, "only the used prefix"
        assert table.dtype == torch.int32 and table.tolist() == wt.tolist()
        assert all(np.array_equal(g, a) for g, a in zip(pixels(packed, table, C_), want))
        assert lab.tolist() == [y for _, y in ds[seen:seen + n]]
        assert boxes.shape == (n, 4) and flips.shape == (n,)
        b = boxes.numpy()
        hw = table.numpy()[:, 1:3]
        assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 2] <= hw[:, 0]).all() and (b[:, 1] + b[:, 3] <= hw[:, 1]).all()
        seen += n
    assert seen == 10


def test_oversize_error_names_the_sample_and_crop_is_centred():
    ds = dataset(6)
    ld = NativeImageLoader(ds, 3, (0, 0), CPU, out_hw=(32, 32), ragged_max_hw=(48, 60))
    with pytest.raises(ValueError, match=r"sample 2: 64 x 36 exceeds"):
        list(ld)
    ld = NativeImageLoader(ds, 3, (0, 0), CPU, out_hw=(32, 32), ragged_max_hw=(48, 60), oversize="crop")
    batches = list(ld)
    packed, _, _, _, table = batches[0]
    assert table[:, 1:3].tolist() == [[40, 52], [33, 47], [48, 36]]
    assert np.array_equal(pixels(packed, table, 3)[2], ds[2][0][8:56])  # (64 - 48) // 2 rows off the top
    packed, _, _, _, table = batches[1]
    assert table[:, 1:3].tolist() == [[48, 48], [37, 60], [1, 1]]
    assert np.array_equal(pixels(packed, table, 3)[1], ds[4][0][:, 5:65])
    for kw in (dict(oversize="squash", ragged_max_hw=(8, 8)), dict(oversize="crop"), dict(ragged_max_hw=(8, 0)),
               dict(ragged_max_hw=(64, 72), device_cache=True)):
        with pytest.raises(ValueError):
            NativeImageLoader(ds, 3, (0, 0), CPU, out_hw=(32, 32), **kw)


@pytest.mark.skipif(not _ext.available(), reason="native extension not built")
@pytest.mark.parametrize("encoding", ["pil", "ndarray"])
def test_gather_ragged_equals_the_python_path(tmp_path, encoding):
    from dbx_distributed_pytorch_examples_amd.data.mds import MDSWriter, StreamingDataset, write_image_dataset_mds
    sizes = SIZES if encoding == "pil" else [(9, 11)]
    ds = dataset(11, sizes=sizes)
    out = str(tmp_path / "mds")
    if encoding == "pil":
        write_image_dataset_mds(ds, out, size_limit=20000)  # several shards
    else:
        with MDSWriter(out, {"image": "ndarray:uint8:9,11,3", "label": "int"}) as w:
            for a, y in ds:
                w.write({"image": a, "label": y})
    sd = StreamingDataset(local=out, shuffle=False)
    ids = np.array([7, 0, 3, 10, 5, 2], np.int64)
    kw = dict(out_hw=(32, 32), ragged_max_hw=(48, 60), oversize="crop", drop_last=False, indices_fn=lambda e: ids)
    native = NativeImageLoader(sd, 4, (0, 0), CPU, **kw)
    assert native.native is not None and native.pool is None
    python = NativeImageLoader(ds, 4, (0, 0), CPU, **kw)
    nb = 0
    for a, b in zip(native, python):
        assert torch.equal(a[4], b[4]), "the table"
        assert a[0].numel() == b[0].numel()
        assert all(np.array_equal(x, y) for x, y in zip(pixels(a[0], a[4], 3), pixels(b[0], b[4], 3)))
        assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
        nb += 1
    assert nb == 2
    if encoding == "pil":
        strict = NativeImageLoader(sd, 4, (0, 0), CPU, **{**kw, "oversize": "error"})
        with pytest.raises(ValueError, match=r"sample 2: 64 x 36 exceeds"):
            list(strict)
        rd = sd.native_reader()
        small, tab = torch.zeros(64, dtype=torch.uint8), torch.zeros(6, 4, dtype=torch.int32)
        with pytest.raises(RuntimeError, match="ragged batch of more than 64 bytes"):
            rd.gather_ragged(ids, small.data_ptr(), small.numel(), tab.data_ptr(), 0, 64, 72, 3)
        assert not small.any(), "nothing is copied into an arena the batch does not fit"


# ---------------------------------------------------------------------------------------------
MODES = [AugmentSpec(), AugmentSpec(mode="random_resized_crop", hflip=True),
         AugmentSpec(mode="random_resized_crop", scale=(0.9, 1.0), ratio=(0.9, 1.1)),  # (the centre fallback)
         AugmentSpec(mode="random_crop", pad=4, hflip=True), AugmentSpec(mode="center_crop"),
         AugmentSpec(mode="resize_center_crop")]


@pytest.mark.parametrize("spec", MODES, ids=lambda s: f"{s.mode}-{s.scale[0]}")
@pytest.mark.parametrize("hw", [(32, 32), (256, 341), (500, 120), (64, 300)])
def test_sample_boxes_ints_against_constant_arrays(spec, hw):
    n, (h, w) = 33, hw
    ho = wo = 32
    a = sample_boxes(n, h, w, ho, wo, spec, random.Random(5))
    b = sample_boxes(n, np.full(n, h), np.full(n, w, dtype=np.int32), ho, wo, spec, random.Random(5))
    assert a[0].dtype == b[0].dtype == np.float32 and a[0].shape == (n, 4)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_sample_boxes_per_sample_sizes():
    hs, ws = np.array([40, 33, 64, 1, 500]), np.array([52, 47, 36, 1, 120])
    bx, fl = sample_boxes(5, hs, ws, 32, 32, AugmentSpec(mode="random_resized_crop", hflip=True), random.Random(1))
    assert (bx[:, 0] >= 0).all() and (bx[:, 1] >= 0).all() and (bx[:, 2] >= 1).all() and (bx[:, 3] >= 1).all()
    assert (bx[:, 0] + bx[:, 2] <= hs).all() and (bx[:, 1] + bx[:, 3] <= ws).all()
    near = AugmentSpec(mode="random_resized_crop", scale=(0.9, 1.0), ratio=(0.9, 1.1))
    bx, _ = sample_boxes(5, hs, ws, 32, 32, near, random.Random(1))
    # 500 x 120 and 64 x 36: no near-square box of 90 % of the area fits, the centre crop clamped to the ratio range
    assert np.array_equal(bx[4], [(500 - 133) // 2, 0, 133, 120]) and np.array_equal(bx[2], [(64 - 40) // 2, 0, 40, 36])
    assert np.array_equal(bx[3], [0, 0, 1, 1])
    full, _ = sample_boxes(5, hs, ws, 32, 32, AugmentSpec(), random.Random(1))
    assert np.array_equal(full, np.stack([0 * hs, 0 * ws, hs, ws], 1))


def test_resize_center_crop():
    """torchvision's Resize(shorter side) + CenterCrop: the centred square of round(crop_frac * min(h, w))."""
    hs, ws = np.array([256, 341, 40, 7, 224]), np.array([341, 256, 40, 300, 225])
    for frac in (0.875, 1.0):
        bx, fl = sample_boxes(5, hs, ws, 224, 224, AugmentSpec(mode="resize_center_crop", crop_frac=frac),
                              random.Random(0))
        side = np.rint(frac * np.minimum(hs, ws))
        assert np.array_equal(bx[:, 2], side) and np.array_equal(bx[:, 3], side) and not fl.any()
        assert np.array_equal(bx[:, 0], (hs - side) // 2) and np.array_equal(bx[:, 1], (ws - side) // 2)
    bx, _ = sample_boxes(2, 256, 341, 224, 224, AugmentSpec(mode="resize_center_crop"), random.Random(0))
    assert bx.tolist() == [[16.0, 58.0, 224.0, 224.0]] * 2
    # the existing mode is untouched: both sides scaled
    bx, _ = sample_boxes(1, 256, 341, 224, 224, AugmentSpec(mode="center_crop"), random.Random(0))
    assert bx.tolist() == [[16.0, 21.0, 224.0, 298.0]]


def test_a_uniform_dataset_draws_the_dense_loaders_boxes():
    ds = dataset(12, sizes=[(40, 52)])
    spec = AugmentSpec(mode="random_resized_crop", hflip=True)
    dense = NativeImageLoader(ds, 4, (40, 52), CPU, augment=spec, out_hw=(32, 32), seed=9)
    ragged = NativeImageLoader(ds, 4, (0, 0), CPU, augment=spec, out_hw=(32, 32), seed=9, ragged_max_hw=(40, 52))
    for e in range(2):
        dense.set_epoch(e)
        ragged.set_epoch(e)
        for a, b in zip(dense, ragged):
            assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and torch.equal(a[1], b[1])
            assert all(np.array_equal(x, y) for x, y in zip(pixels(b[0], b[4], 3), a[0].numpy()))


# ---------------------------------------------------------------------------------------------
def test_config_options():
    d = C.TrainConfig().data
    assert (d.ragged, tuple(d.ragged_max_hw), d.ragged_oversize) == (False, (512, 512), "error")
    assert C.ragged_options(d) == {}
    cfg = C.load_config(overrides=["data.ragged=true", "data.ragged_max_hw=[300,400]", "data.ragged_oversize=crop"])
    assert C.ragged_options(cfg.data) == dict(ragged_max_hw=(300, 400), oversize="crop")
    C.validate_data(cfg.data)
    for k, v in (("ragged_max_hw", (256, 256)), ("ragged_oversize", "crop")):
        d = C.TrainConfig().data
        setattr(d, k, v)
        with pytest.raises(ValueError, match="data.ragged"):
            C.validate_data(d)
    for k, v in (("ragged_max_hw", (0, 8)), ("ragged_max_hw", (8,)), ("ragged_max_hw", 512), ("ragged_oversize", "squash"),
                 ("ragged", 1)):
        d = C.TrainConfig().data
        d.ragged = True
        setattr(d, k, v)
        with pytest.raises(ValueError):
            C.validate_data(d)
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs")
    rg = C.load_config(os.path.join(root, "resnet50_imagenet_8192_recipe_ragged.yaml"))
    base = C.load_config(os.path.join(root, "resnet50_imagenet_8192_recipe.yaml"))
    assert rg.data.ragged and rg.data.dataset == "mds" and not base.data.ragged
    C.validate_train(rg)
    assert rg.optim == base.optim and rg.batch_size == base.batch_size and rg.data.mixup_alpha == base.data.mixup_alpha


def test_write_time_resize(tmp_path):
    from dbx_distributed_pytorch_examples_amd.data.mds import StreamingDataset, write_image_dataset_mds
    ds = dataset(4, sizes=[(40, 52), (64, 36), (32, 32)])
    write_image_dataset_mds(ds, str(tmp_path / "m"), shorter_side=32)
    sd = StreamingDataset(local=str(tmp_path / "m"), shuffle=False)
    got = [np.asarray(sd[i]["image"]).shape[:2] for i in range(4)]
    assert got == [(32, 41), (56, 32), (32, 32), (32, 41)], "the shorter side is 32, the aspect ratio kept"
    with pytest.raises(ValueError):
        write_image_dataset_mds(ds, str(tmp_path / "n"), shorter_side=0)


def png_folder(root, per_class=4):
    rs = np.random.default_rng(0)
    for split, n in (("train", per_class), ("val", 3)):
        for c in range(2):
            os.makedirs(os.path.join(root, split, f"c{c}"))
            for i in range(n):
                h, w = SIZES[(i + 2 * c) % 5]
                Image.fromarray(rs.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(
                    os.path.join(root, split, f"c{c}", f"{i}.png"))


def test_train_on_a_folder_of_pngs_of_several_sizes(tmp_path, monkeypatch):
    """One epoch of the native step on the CPU path, images read at their own sizes: a finite loss, and validation
    over a short last batch. Without ``data.ragged`` the loader stops at the first image of another size."""
    from dbx_distributed_pytorch_examples_amd.data.datasets import build_dataset
    from dbx_distributed_pytorch_examples_amd.train import engine as E
    monkeypatch.setenv("DBX_FORCE_CPU", "1")
    root = str(tmp_path)
    png_folder(root)

    def cfg(**data):
        c = C.TrainConfig(model="resnet18", num_classes=2, batch_size=4, epochs=1, engine="native")
        c.data.dataset, c.data.root, c.data.image_size, c.data.num_workers = "folder", root, 32, 2
        c.optim.lr = 0.01
        for k, v in data.items():
            setattr(c.data, k, v)
        return c

    r = E.train(cfg(ragged=True, ragged_max_hw=(64, 72)), eval_dataset=build_dataset("folder", root, False),
                log_mlflow=False)
    rec = r.history[-1]
    assert r.engine == "native" and r.steps == 2
    assert math.isfinite(rec["train_loss"]) and rec["train_loss"] > 0 and rec["val_samples"] == 6
    assert math.isfinite(rec["val_loss"])
    r = E.train(cfg(ragged=True, ragged_max_hw=(64, 72), augment=False), log_mlflow=False)
    assert math.isfinite(r.history[-1]["train_loss"])
    with pytest.raises(ValueError, match="exceeds ragged_max_hw"):
        E.train(cfg(ragged=True, ragged_max_hw=(48, 72)), log_mlflow=False)
    with pytest.raises(ValueError, match="loader expects"):
        E.train(cfg(), log_mlflow=False)


def test_train_refuses_ragged_on_the_other_engines(monkeypatch):
    from dbx_distributed_pytorch_examples_amd.engine.autograd_trainer import AutogradTrainer
    from dbx_distributed_pytorch_examples_amd.engine.frozen_trainer import FrozenFeatureTrainer
    from dbx_distributed_pytorch_examples_amd.engine.native_module import native_module
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import OptimConfig
    from dbx_distributed_pytorch_examples_amd.models import FrozenBackboneClassifier, build_model
    from dbx_distributed_pytorch_examples_amd.train import engine as E
    monkeypatch.setenv("DBX_FORCE_CPU", "1")
    boom = lambda *a, **k: (_ for _ in ()).throw(AssertionError("built a runner"))  # noqa: E731
    monkeypatch.setattr(E, "_Autograd", boom)
    monkeypatch.setattr(E, "_Native", boom)
    c = C.TrainConfig(model="resnet18", num_classes=10, batch_size=4, max_steps=1)
    c.data.image_size, c.data.train_samples, c.data.ragged = 32, 8, True
    with pytest.raises(ValueError, match="autograd engine"):
        E.train(c, log_mlflow=False)
    monkeypatch.setattr(E, "_pick_engine", lambda *a: "native")
    with pytest.raises(ValueError, match="frozen-backbone"):
        E.train(c, model=FrozenBackboneClassifier("resnet18", num_classes=10), log_mlflow=False)
    with pytest.raises(ValueError, match="src_ragged"):
        AutogradTrainer(build_model("resnet18", num_classes=10), CPU, OptimConfig(), src_ragged=(64, 64))
    with pytest.raises(ValueError, match="src_ragged"):
        FrozenFeatureTrainer(FrozenBackboneClassifier("resnet18", num_classes=10), 4, (32, 32), CPU, OptimConfig(),
                             src_ragged=(64, 64))
    with pytest.raises(ValueError, match="src_ragged"):
        native_module(build_model("resnet18", num_classes=10), 4, (32, 32), CPU, src_ragged=(64, 64))
