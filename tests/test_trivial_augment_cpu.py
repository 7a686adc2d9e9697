"""TrivialAugmentWide without a GPU: the numpy definition (``ops/reference.py``) against Pillow -- the library
torchvision calls for these operations on PIL images -- the Pillow transform of ``data/transforms.py``, the
sampler, the trainer's wiring on the CPU path, the config and every refusal above the kernel wrappers."""
import math
import os

import numpy as np
import pytest
import torch

from dbx_distributed_pytorch_examples_amd.engine import mix as M
from dbx_distributed_pytorch_examples_amd.ops import kernels as K
from dbx_distributed_pytorch_examples_amd.ops import reference as R

CPU = torch.device("cpu")
SHAPES = [(16, 16), (24, 40), (32, 32)]
shapes = pytest.mark.parametrize("H,W", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
ANGLES = (4.5, 40.5, -100.3, 67.5, 121.5)
# (kind, magnitude): every kind but Rotate, at the extremes of each magnitude and one value inside
EXACT = ([(0, 0.0)]
         + [(k, m) for k in (1, 2) for m in (0.99, -0.99, 0.33)]
         + [(k, t) for k in (3, 4) for t in (32.0, -32.0, 7.0)]
         + [(k, p) for k in (6, 7, 8, 9) for p in (0.01, 1.0, 1.99, 0.34, 1.33)]
         + [(10, b) for b in (2.0, 8.0, 5.0)]
         + [(11, t) for t in (0.0, 255.0, 127.5, 8.5)]
         + [(12, 0.0), (13, 0.0)])


def images(H, W):
    rs = np.random.default_rng(H * 100 + W)
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = np.stack([(yy * 7 + xx * 3) % 256, (xx * 5) % 251, (yy * xx) % 256], -1)
    return {"random": rs.integers(0, 256, (H, W, 3)).astype(np.uint8),
            "narrow": rs.integers(40, 200, (H, W, 3)).astype(np.uint8),
            "ramp": ramp.astype(np.uint8),
            "constant": np.full((H, W, 3), 77, np.uint8),                                     # step == 0, lo == hi
            "per-channel": np.ascontiguousarray(np.broadcast_to(np.array([10, 200, 77], np.uint8), (H, W, 3))),
            "two-level": np.where(rs.integers(0, 2, (H, W, 3)) > 0, 230, 20).astype(np.uint8)}


# ---------------------------------------------------------------------------------------------
# 1. the definition == Pillow
# ---------------------------------------------------------------------------------------------
@shapes
def test_definition_equals_pillow(H, W):
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageEnhance, ImageOps
    pil = {6: ImageEnhance.Brightness, 7: ImageEnhance.Color, 8: ImageEnhance.Contrast, 9: ImageEnhance.Sharpness}
    for name, a in images(H, W).items():
        im = Image.fromarray(a)
        for kind, mag in EXACT:
            got = R.ta_apply_image(a, M.ta_row(kind, mag, H, W))
            if kind == 0:
                want = im
            elif kind == 1:
                want = im.transform((W, H), Image.AFFINE, (1, mag, 0, 0, 1, 0), Image.NEAREST, fillcolor=0)
            elif kind == 2:
                want = im.transform((W, H), Image.AFFINE, (1, 0, 0, mag, 1, 0), Image.NEAREST, fillcolor=0)
            elif kind == 3:
                want = im.transform((W, H), Image.AFFINE, (1, 0, -mag, 0, 1, 0), Image.NEAREST, fillcolor=0)
            elif kind == 4:
                want = im.transform((W, H), Image.AFFINE, (1, 0, 0, 0, 1, -mag), Image.NEAREST, fillcolor=0)
            elif kind in pil:
                want = pil[kind](im).enhance(float(np.float32(mag)))
            elif kind == 10:
                want = ImageOps.posterize(im, int(mag))
            elif kind == 11:
                want = ImageOps.solarize(im, mag)
            elif kind == 12:
                want = ImageOps.autocontrast(im)
            else:
                want = ImageOps.equalize(im)
            assert np.array_equal(got, np.asarray(want)), (name, R.TA_NAMES[kind], mag)
    if W == 32:  # t = +-32 empties a 32-wide image
        a = images(H, W)["random"]
        assert not R.ta_apply_image(a, M.ta_row(3, 32.0, H, W)).any()


def _near_integer(row, H, W):
    """Pixels whose float64 source coordinate lies within 1e-3 of an integer (Pillow walks the image in
    16.16 fixed point, so only there can its floor differ)."""
    co = [float(v) for v in np.asarray(row[2:8]).view(np.float32)]
    yy, xx = np.mgrid[0:H, 0:W]
    xi = co[0] * (xx + 0.5) + co[1] * (yy + 0.5) + co[2]
    yi = co[3] * (xx + 0.5) + co[4] * (yy + 0.5) + co[5]
    return np.minimum(np.abs(xi - np.round(xi)), np.abs(yi - np.round(yi))) < 1e-3


@pytest.mark.parametrize("angle", ANGLES)
@shapes
def test_rotation_equals_pillow_away_from_pixel_edges(H, W, angle):
    """Equal at every pixel whose float64 source coordinates are at least 1e-3 from an integer; the excluded
    share is <= 2 % (the definition alone reads at most 1.56 % on these shapes), asserted first."""
    Image = pytest.importorskip("PIL.Image")
    a = images(H, W)["random"]
    row = M.ta_row(5, angle, H, W)
    near = _near_integer(row, H, W)
    print(f"rotation {angle} at {H}x{W}: excluded share {near.mean():.4f}")
    assert near.mean() <= 0.02
    got = R.ta_apply_image(a, row)
    want = np.asarray(Image.fromarray(a).rotate(angle, Image.NEAREST))
    assert np.array_equal(got[~near], want[~near])
    from dbx_distributed_pytorch_examples_amd.data.transforms import TrivialAugmentWide
    again = np.asarray(TrivialAugmentWide.apply(a, row))
    assert np.array_equal(got[~near], again[~near])


@shapes
def test_pillow_transform_takes_the_same_table(H, W):
    """``data.transforms.TrivialAugmentWide.apply`` with a fixed table: the definition's pixels."""
    pytest.importorskip("PIL.Image")
    from dbx_distributed_pytorch_examples_amd.data.transforms import Compose, TrivialAugmentWide
    for name, a in images(H, W).items():
        for kind, mag in EXACT:
            row = M.ta_row(kind, mag, H, W)
            assert np.array_equal(np.asarray(TrivialAugmentWide.apply(a, row)), R.ta_apply_image(a, row)), (name, kind, mag)
    import random
    random.seed(3)
    t = Compose([TrivialAugmentWide()])
    a = images(H, W)["random"]
    outs = [np.asarray(t(a)) for _ in range(40)]
    assert all(o.shape == a.shape and o.dtype == np.uint8 for o in outs)
    assert sum(not np.array_equal(o, a) for o in outs) > 20
    with pytest.raises(ValueError):
        TrivialAugmentWide(num_bins=1)


# ---------------------------------------------------------------------------------------------
# 6. the sampler
# ---------------------------------------------------------------------------------------------
def test_sampler_is_uniform_over_kinds_bins_and_signs():
    n, bins = 14 * 31 * 2000, 31
    rs = np.random.default_rng(17)
    idx_probe = np.random.default_rng(17)
    kind, rows = M.sample_trivial_augment(rs, n, 32, 32, bins)
    k2, i2, s2 = idx_probe.integers(14, size=n), idx_probe.integers(bins, size=n), idx_probe.integers(2, size=n)
    assert np.array_equal(kind, k2), "three vectorised draws: integers(14, n), integers(num_bins, n), integers(2, n)"
    assert rs.integers(1 << 30) == idx_probe.integers(1 << 30), "and nothing else"
    assert kind.dtype == np.int32 and rows.dtype == np.int32 and rows.shape == (n, 8) and np.array_equal(rows[:, 0], kind)
    for counts, m in ((np.bincount(kind, minlength=14), 14), (np.bincount(i2, minlength=bins), bins)):
        assert len(counts) == m and counts.min() > 0
        p = 1.0 / m
        assert np.abs(counts / n - p).max() <= 5 * math.sqrt(p * (1 - p) / n)
    par = rows[:, 1:].view(np.float32)
    signed = np.isin(kind, (1, 2, 3, 4, 5, 6, 7, 8, 9)) & (i2 > 0)
    neg = np.where(kind <= 2, par[:, 2] + par[:, 4] < 0, np.where(kind <= 4, par[:, 3] + par[:, 6] > 0,
                   np.where(kind == 5, par[:, 2] > 0, par[:, 0] < 1)))
    assert np.array_equal(neg[signed], s2[signed] == 1), "the third draw is the sign of every signed magnitude"
    ns = int(signed.sum())
    assert abs(float(neg[signed].mean()) - 0.5) <= 5 * math.sqrt(0.25 / ns)
    bits = par[kind == 10, 0]
    assert set(bits.tolist()) == {2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0}
    t = np.concatenate([par[kind == 3, 3], par[kind == 4, 6]])
    assert np.array_equal(t, np.rint(t)) and np.abs(t).max() == 32 and set(np.abs(t).tolist()) == {
        float(int(32 * i / 30)) for i in range(31)}
    p = par[(kind >= 6) & (kind <= 9), 0]
    assert abs(p.min() - 0.01) < 1e-6 and abs(p.max() - 1.99) < 1e-6
    thr = par[kind == 11, 0]
    assert thr.min() == 0.0 and thr.max() == 255.0
    m = np.concatenate([par[kind == 1, 2], par[kind == 2, 4]])
    assert abs(m.min() + 0.99) < 1e-6 and abs(m.max() - 0.99) < 1e-6


def test_table_rows_match_the_scalar_builder():
    for bins in (31, 2, 7):
        for H, W in ((32, 32), (24, 40)):
            kind, idx, sign = (a.ravel() for a in np.meshgrid(np.arange(14), np.arange(bins), np.arange(2), indexing="ij"))
            rows = M.ta_table(kind, idx, sign, H, W, bins).view(np.float32)
            for j in range(len(kind)):
                k, i, s = int(kind[j]), int(idx[j]), int(sign[j])
                want = M.ta_row(k, M.ta_magnitude(k, i, s, bins), H, W)
                assert int(rows[j, :1].view(np.int32)[0]) == k
                assert np.array_equal(rows[j, 1:], want[1:].view(np.float32)), (k, i, s)  # (-0.0 == 0.0)
    # the rotation matrix: Pillow's, in double, about (W / 2, H / 2)
    r = M.ta_row(5, 40.5, 24, 40)[1:].view(np.float32)
    al = -math.radians(40.5)
    C, S = round(math.cos(al), 15), round(math.sin(al), 15)
    want = (0.0, C, S, 20.0 - C * 20.0 - S * 12.0, -S, C, 12.0 + S * 20.0 - C * 12.0)
    assert np.allclose(r, np.float32(want), rtol=0, atol=4e-6)
    assert M.ta_row(5, 90.0, 32, 32)[1:].view(np.float32).tolist() == [0.0, 0.0, -1.0, 32.0, 1.0, 0.0, 0.0]
    with pytest.raises(ValueError):
        M.ta_row(14, 0.0, 8, 8)


@pytest.mark.parametrize("kw", [dict(cutmix_alpha=1.0), dict(mixup_alpha=0.2, cutmix_alpha=1.0, mix_prob=0.7, erase_prob=0.5),
                                dict()])
def test_option_leaves_the_earlier_draws_identical(kw):
    a = M.MixSampler(np.random.default_rng(9), 8, 32, 32, **kw)
    b = M.MixSampler(np.random.default_rng(9), 8, 32, 32, auto_augment="ta_wide", **kw)
    probe = np.random.default_rng(9)
    for _ in range(20):
        da, db = a.sample(), b.sample()
        assert da.ta is None and db.ta.shape == (8, 8) and db["ta"] is db.ta
        assert (da.kind, da.lam, da.blend, da.box) == (db.kind, db.lam, db.blend, db.box)
        assert np.array_equal(da.perm, db.perm)
        assert (da.erase is None and db.erase is None) or np.array_equal(da.erase, db.erase)
        # sampler b drew exactly the table after what a drew
        st = a.rng.bit_generator.state
        probe.bit_generator.state = st
        assert np.array_equal(M.sample_trivial_augment(probe, 8, 32, 32)[1], db.ta)
        a.rng.bit_generator.state = b.rng.bit_generator.state  # keep the two streams aligned for the next step


# ---------------------------------------------------------------------------------------------
# the trainer on the CPU path
# ---------------------------------------------------------------------------------------------
def _trainer(model="resnet18", **kw):
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer
    from dbx_distributed_pytorch_examples_amd.models import build_model
    torch.manual_seed(0)
    m = build_model(model, num_classes=10) if isinstance(model, str) else model
    return NativeTrainer(m, 4, (32, 32), CPU, **kw)


def test_trainer_wiring_on_cpu():
    """The program's table follows the host draw, the input is the pipeline's output for it, evaluation never
    augments, and the summary names the option."""
    tr = _trainer(auto_augment="ta_wide", mixup_alpha=0.2, cutmix_alpha=1.0, erase_prob=0.5, erase_mode="pixel", seed=2)
    p = tr.prog
    N = p.N
    assert p.mix_arena.numel() == 13 * N + 6 and not p.ta_ops.any() and tuple(p.ta_T.shape) == (N, 32, 32, 4)
    img = torch.randint(0, 256, (4, 32, 32, 3), dtype=torch.uint8)
    lab = torch.randint(0, 10, (4,))
    kinds = set()
    for i in range(5):
        tr.step(img, lab)
        d = tr.last_mix
        kinds.update(d["ta"][:, 0].tolist())
        assert p.ta_ops.tolist() == d.ta.tolist() and p.erase_box.tolist() == d.erase.tolist()
        assert p.mix_perm.tolist() == d.perm.tolist() and float(p.mix_blend) == d.blend
        want = torch.empty_like(p.x4)
        work = torch.zeros(K.ta_work_words(N, 32, 32), dtype=torch.int32)
        K.trivial_augment_u8(p.img_u8, want, p.boxes, p.mean_t.tolist(), p.std_t.tolist(), p.flip,
                             torch.from_numpy(d.ta), work, perm=p.mix_perm, mixbox=p.mix_box, blend=p.mix_blend,
                             erase=p.erase_box, erase_mode="pixel", erase_rng=(p.erase_seed, p.erase_off))
        assert torch.equal(p.x4, want)
    assert len(kinds) > 3
    tr.evaluate_batch(img, lab)
    plain = torch.empty_like(p.x4)
    K.augment_u8(p.img_u8, plain, p.boxes, p.mean_t.tolist(), p.std_t.tolist(), p.flip)
    assert torch.equal(p.x4, plain)
    s = tr.mix_summary()
    assert s["auto_augment"] == "ta_wide" and s["kernel"] == "trivial_augment_u8" and s["ta_num_bins"] == 31


def test_option_alone_uses_the_arena_and_off_allocates_nothing():
    tr = _trainer(auto_augment="ta_wide", ta_num_bins=5, seed=1)
    p = tr.prog
    assert p.mix_arena is not None and p.ta_ops is not None and p.ta_work.numel() == K.ta_work_words(4, 32, 32)
    img, lab = torch.randint(0, 256, (4, 32, 32, 3), dtype=torch.uint8), torch.randint(0, 10, (4,))
    tr.step(img, lab)
    d = tr.last_mix
    assert d.kind == "none" and d.erase is None and p.ta_ops.tolist() == d.ta.tolist()
    assert tr._mix_ring[0][0].numel() == 13 * 4 + 6, "a ring slot sized to the arena"
    off = _trainer(seed=1)
    assert off.prog.ta_ops is None and off.prog.ta_work is None and off.prog.mix_arena is None and off._mix is None
    s = off.mix_summary()
    assert s["kernel"] == "augment_u8" and s["auto_augment"] is None
    assert _trainer(mixup_alpha=0.2).prog.mix_arena.numel() == 5 * 4 + 6, "without the option the arena keeps its size"
    assert _trainer(mixup_alpha=0.2).mix_summary()["kernel"] == "augment_mix_u8"


# ---------------------------------------------------------------------------------------------
# 8. config and refusals
# ---------------------------------------------------------------------------------------------
BAD = [dict(auto_augment="ta"), dict(auto_augment="randaugment"), dict(auto_augment="ta_wide", ta_num_bins=1),
       dict(ta_num_bins=0), dict(auto_augment="ta_wide", ta_num_bins=2.5)]


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_bad_values_raise(kw, monkeypatch):
    from dbx_distributed_pytorch_examples_amd import config as C
    from dbx_distributed_pytorch_examples_amd.train import engine as E
    with pytest.raises(ValueError):
        M.validate_auto_augment(**kw)
    with pytest.raises(ValueError):
        _trainer(**kw)
    cfg = C.TrainConfig(model="resnet18", num_classes=10, batch_size=4, max_steps=1)
    cfg.data.image_size, cfg.data.train_samples = 32, 8
    for k, v in kw.items():
        setattr(cfg.data, k, v)
    with pytest.raises(ValueError):
        C.validate_data(cfg.data)
    monkeypatch.setenv("DBX_FORCE_CPU", "1")
    monkeypatch.setattr(E, "_Autograd", lambda *a, **k: (_ for _ in ()).throw(AssertionError("built a runner")))
    with pytest.raises(ValueError):
        E.train(cfg, log_mlflow=False)


def test_trainers_refuse_what_they_cannot_do():
    from dbx_distributed_pytorch_examples_amd.engine.autograd_trainer import AutogradTrainer
    from dbx_distributed_pytorch_examples_amd.engine.frozen_trainer import FrozenFeatureTrainer
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import OptimConfig
    from dbx_distributed_pytorch_examples_amd.models import FrozenBackboneClassifier, build_model
    with pytest.raises(ValueError, match="auto_augment"):
        AutogradTrainer(build_model("resnet18", num_classes=10), CPU, OptimConfig(), auto_augment="ta_wide")
    with pytest.raises(ValueError, match="auto_augment"):
        FrozenFeatureTrainer(FrozenBackboneClassifier("resnet18", num_classes=10), 4, (32, 32), CPU, OptimConfig(),
                             auto_augment="ta_wide")
    gray = build_model("resnet18", num_classes=10, in_channels=1)
    with pytest.raises(ValueError, match="3-channel"):
        _trainer(gray, auto_augment="ta_wide")
    from dbx_distributed_pytorch_examples_amd.engine.program import ResNetProgram
    prog = ResNetProgram(gray, 4, (32, 32), CPU)
    with pytest.raises(ValueError, match="3-channel"):
        prog.enable_mix(ta=True)


def test_train_refuses_the_other_engines(monkeypatch):
    """``auto_augment`` is refused, never ignored, where the native step does not run: the autograd engine
    (here: no GPU), the frozen-backbone trainer, a 1-channel model."""
    from dbx_distributed_pytorch_examples_amd import config as C
    from dbx_distributed_pytorch_examples_amd.models import FrozenBackboneClassifier, build_model
    from dbx_distributed_pytorch_examples_amd.train import engine as E
    monkeypatch.setenv("DBX_FORCE_CPU", "1")
    boom = lambda *a, **k: (_ for _ in ()).throw(AssertionError("built a runner"))  # noqa: E731
    monkeypatch.setattr(E, "_Autograd", boom)
    monkeypatch.setattr(E, "_Native", boom)

    def cfg(**kw):
        c = C.TrainConfig(model="resnet18", num_classes=10, batch_size=4, max_steps=1, **kw)
        c.data.image_size, c.data.train_samples, c.data.auto_augment = 32, 8, "ta_wide"
        return c

    with pytest.raises(ValueError, match="autograd engine"):
        E.train(cfg(), log_mlflow=False)
    with pytest.raises(ValueError, match="autograd engine"):
        E.train(cfg(engine="autograd"), log_mlflow=False)
    monkeypatch.setattr(E, "_pick_engine", lambda *a: "native")
    with pytest.raises(ValueError, match="frozen-backbone"):
        E.train(cfg(), model=FrozenBackboneClassifier("resnet18", num_classes=10), log_mlflow=False)
    with pytest.raises(ValueError, match="3-channel"):
        E.train(cfg(), model=build_model("resnet18", num_classes=10, in_channels=1), log_mlflow=False)


def test_config_loads_and_reaches_the_trainer():
    from dbx_distributed_pytorch_examples_amd import config as C
    cfg = C.load_config(overrides=["data.auto_augment=ta_wide", "data.ta_num_bins=11"])
    assert C.auto_augment_options(cfg.data) == dict(auto_augment="ta_wide", ta_num_bins=11)
    assert C.auto_augment_options(C.TrainConfig().data) == dict(auto_augment=None, ta_num_bins=31)
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs")
    ta = C.load_config(os.path.join(root, "resnet50_imagenet_8192_recipe_ta.yaml"))
    base = C.load_config(os.path.join(root, "resnet50_imagenet_8192_recipe.yaml"))
    assert ta.data.auto_augment == "ta_wide" and ta.data.ta_num_bins == 31 and base.data.auto_augment is None
    C.validate_data(ta.data)
    ta.data.auto_augment = None
    assert C.to_dict(ta) == C.to_dict(base), "the recipe config plus the one option"
