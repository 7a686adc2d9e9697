"""RandAugment and the AutoAugment ImageNet policy without a GPU: the magnitude space against ``torch.linspace``,
the policy table, the sampler's draws, the fold of the numpy definition (``ops/reference.py``) against Pillow
through ``data/transforms.py``, the trainer's wiring on the CPU path, the config and every refusal above the
kernel wrappers."""
import os

import numpy as np
import pytest
import torch

from dbx_distributed_pytorch_examples_amd.engine import mix as M
from dbx_distributed_pytorch_examples_amd.ops import kernels as K
from dbx_distributed_pytorch_examples_amd.ops import reference as R
from test_trivial_augment_cpu import _near_integer, _trainer, images

CPU = torch.device("cpu")
SIZES = (32, 64, 224)


# ---------------------------------------------------------------------------------------------
# the magnitude space
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_bins", [31, 10])
def test_magnitudes_against_torch_linspace(num_bins):
    """Every entry of the table, element for element: x_i is the i-th entry of the float32 linspace, read as one
    Python float, as torchvision does."""
    nb = num_bins
    post = 8 - (torch.arange(nb) / ((nb - 1) / 4)).round().int()
    for Ho in SIZES:
        for Wo in SIZES:
            lin = {1: torch.linspace(0.0, 0.3, nb), 2: torch.linspace(0.0, 0.3, nb),
                   3: torch.linspace(0.0, 150.0 / 331.0 * Wo, nb), 4: torch.linspace(0.0, 150.0 / 331.0 * Ho, nb),
                   5: torch.linspace(0.0, 30.0, nb), 11: torch.linspace(255.0, 0.0, nb)}
            for k in (6, 7, 8, 9):
                lin[k] = torch.linspace(0.0, 0.9, nb)
            assert all(v.dtype == torch.float32 for v in lin.values())
            kind, idx, sign = (a.ravel() for a in np.meshgrid(np.arange(14), np.arange(nb), np.arange(2), indexing="ij"))
            rows = M.ra_table(kind, idx, sign, Ho, Wo, nb)
            for j in range(len(kind)):
                k, i, s = int(kind[j]), int(idx[j]), int(sign[j])
                sg = -1.0 if s else 1.0
                if k in (1, 2, 5):
                    want = sg * float(lin[k][i])
                elif k in (3, 4):
                    want = sg * int(lin[k][i])
                elif k in (6, 7, 8, 9):
                    want = 1.0 + sg * float(lin[k][i])
                elif k == 10:
                    want = float(post[i])
                elif k == 11:
                    want = float(lin[k][i])
                else:
                    want = 0.0
                got = M.ra_magnitude(k, i, s, nb, Ho, Wo)
                assert got == want, (R.TA_NAMES[k], i, s, Ho, Wo)
                assert np.array_equal(rows[j].view(np.float32)[1:], M.ta_row(k, want, Ho, Wo).view(np.float32)[1:]) \
                    and rows[j, 0] == k, (k, i, s)  # (-0.0 == 0.0)
    # the ends of the space
    assert M.ra_magnitude(5, nb - 1, 0, nb, 32, 32) == 30.0 and M.ra_magnitude(5, nb - 1, 1, nb, 32, 32) == -30.0
    assert M.ra_magnitude(3, nb - 1, 0, nb, 32, 224) == int(np.float32(150.0 / 331.0 * 224)) == 101
    assert M.ra_magnitude(4, nb - 1, 0, nb, 32, 224) == 14 and M.ra_magnitude(10, nb - 1, 0, nb, 32, 32) == 4.0
    assert M.ra_magnitude(11, 0, 0, nb, 32, 32) == 255.0 and M.ra_magnitude(11, nb - 1, 0, nb, 32, 32) == 0.0
    with pytest.raises(ValueError):
        M.ra_magnitude(14, 0, 0, nb, 32, 32)
    with pytest.raises(ValueError):
        M.ra_magnitude(1, nb, 0, nb, 32, 32)


def test_chain_table_shape_is_kept():
    kind = np.array([[5, 5, 0], [13, 5, 6]])
    rows = M.ra_table(kind, np.full_like(kind, 9), np.array([[0, 1, 0], [0, 0, 1]]), 32, 32, 31)
    assert rows.shape == (2, 3, 8) and rows.dtype == np.int32 and np.array_equal(rows[..., 0], kind)
    assert np.array_equal(rows[0, 0], rows[1, 1]) and not np.array_equal(rows[0, 0], rows[0, 1]), "one matrix per angle"
    assert np.array_equal(rows[0, 1], M.ta_row(5, -9.0, 32, 32))


# ---------------------------------------------------------------------------------------------
# Invert, and the policy table
# ---------------------------------------------------------------------------------------------
def test_invert_is_solarize_at_threshold_zero():
    pytest.importorskip("PIL.Image")
    from PIL import Image, ImageOps
    from dbx_distributed_pytorch_examples_amd.data.transforms import TrivialAugmentWide
    row = M.ta_row(M.aa_kind("Invert"), 0.0, 24, 40)
    assert M.aa_kind("Invert") == 11
    for name, a in images(24, 40).items():
        want = np.asarray(ImageOps.invert(Image.fromarray(a)))
        assert np.array_equal(want, 255 - a)
        assert np.array_equal(np.asarray(TrivialAugmentWide.apply(a, row)), want), name
        assert np.array_equal(R.ta_apply_image(a, row), want), name


# torchvision's AutoAugmentPolicy.IMAGENET: (op, prob, bin), "-" = no magnitude
SPEC = """
 0 Posterize .4 8 | Rotate .6 9          13 Invert .6 - | Equalize 1. -
 1 Solarize .6 5 | AutoContrast .6 -     14 Color .6 4 | Contrast 1. 8
 2 Equalize .8 - | Equalize .6 -         15 Rotate .8 8 | Color 1. 2
 3 Posterize .6 7 | Posterize .6 6       16 Color .8 8 | Solarize .8 7
 4 Equalize .4 - | Solarize .2 4         17 Sharpness .4 7 | Invert .6 -
 5 Equalize .4 - | Rotate .8 8           18 ShearX .6 5 | Equalize 1. -
 6 Solarize .6 3 | Equalize .6 -         19 Color .4 0 | Equalize .6 -
 7 Posterize .8 5 | Equalize 1. -        20 Equalize .4 - | Solarize .2 4
 8 Rotate .2 3 | Solarize .6 8           21 Solarize .6 5 | AutoContrast .6 -
 9 Equalize .6 - | Posterize .4 6        22 Invert .6 - | Equalize 1. -
10 Rotate .8 8 | Color .4 0              23 Color .6 4 | Contrast 1. 8
11 Rotate .4 9 | Equalize .6 -           24 Equalize .8 - | Equalize .6 -
12 Equalize .0 - | Equalize .8 -
"""


def _spec():
    import re
    out = {}
    for m in re.finditer(r"(\d+) (\w+) ([\d.]+) (\S+) \| (\w+) ([\d.]+) (\S+)", SPEC):
        g = m.groups()
        out[int(g[0])] = tuple((g[i], float(g[i + 1]), None if g[i + 2] == "-" else int(g[i + 2])) for i in (1, 4))
    return out


def test_policy_table():
    spec = _spec()
    assert len(M.AA_IMAGENET) == 25 and sorted(spec) == list(range(25))
    for i, sp in enumerate(M.AA_IMAGENET):
        assert tuple(sp) == spec[i], i
        for name, prob, b in sp:
            assert 0 <= M.aa_kind(name) < 14 and 0.0 <= prob <= 1.0
            assert (b is None) == (name in ("Invert", "Equalize", "AutoContrast")) and (b is None or 0 <= b < M.AA_NUM_BINS)
    with pytest.raises(ValueError):
        M.aa_kind("Cutout")
    # prob = 0 never applies, prob = 1 always: at the ends of random()'s range [0, 1) and inside
    us = np.array([0.0, 2.0 ** -53, 0.5, 1.0 - 2.0 ** -53])
    assert not M.aa_applies(us, 0.0).any() and M.aa_applies(us, 1.0).all()
    assert M.aa_applies(us, 0.5).tolist() == [True, True, True, False]
    n = len(us)
    t = M.aa_table([12] * n, np.stack([us, us]), np.zeros((2, n), int), 32, 32)  # Equalize .0 | Equalize .8
    assert not t[0, :, 0].any() and t[1, :, 0].tolist() == [13, 13, 13, 0]
    t = M.aa_table([7] * n, np.stack([us, us]), np.zeros((2, n), int), 32, 32)   # Posterize .8 5 | Equalize 1.
    assert t[0, :, 0].tolist() == [10, 10, 10, 0] and t[1, :, 0].tolist() == [13] * n
    assert t[0, 0].view(np.float32)[1] == M.ra_magnitude(10, 5, 0, 10, 32, 32) == 6.0
    t = M.aa_table([13, 0, 0], np.zeros((2, 3)), [[0, 0, 1], [0, 0, 1]], 32, 64)  # Invert; Posterize 8, Rotate 9 (+, -)
    assert np.array_equal(t[0, 0], M.ta_row(11, 0.0, 32, 64)), "Invert: Solarize at threshold 0"
    assert np.array_equal(t[0, 1], M.ta_row(10, 4.0, 32, 64))
    assert np.array_equal(t[1, 1], M.ta_row(5, 30.0, 32, 64)) and np.array_equal(t[1, 2], M.ta_row(5, -30.0, 32, 64))


# ---------------------------------------------------------------------------------------------
# the sampler
# ---------------------------------------------------------------------------------------------
MIXES = [dict(cutmix_alpha=1.0), dict(mixup_alpha=0.2, cutmix_alpha=1.0, mix_prob=0.7, erase_prob=0.5), dict()]


def _same_draw(da, db):
    assert (da.kind, da.lam, da.blend, da.box) == (db.kind, db.lam, db.blend, db.box)
    assert np.array_equal(da.perm, db.perm)
    assert (da.erase is None and db.erase is None) or np.array_equal(da.erase, db.erase)


@pytest.mark.parametrize("policy", [None, "ta_wide"])
@pytest.mark.parametrize("kw", MIXES)
def test_earlier_policies_draw_what_they_drew(kw, policy):
    """With None / "ta_wide" the new fields at their defaults change no draw: the same sequence as with them
    unset, to the generator's last state (tests/test_trivial_augment_cpu.py pins that sequence itself)."""
    a = M.MixSampler(np.random.default_rng(9), 8, 32, 32, auto_augment=policy, **kw)
    b = M.MixSampler(np.random.default_rng(9), 8, 32, 32, auto_augment=policy, ta_num_bins=31, ra_num_ops=2,
                     ra_magnitude=9, **kw)
    for _ in range(20):
        da, db = a.sample(), b.sample()
        _same_draw(da, db)
        assert (da.ta is None and db.ta is None) if policy is None else (
            da.ta.shape == (8, 8) and np.array_equal(da.ta, db.ta))
    assert a.rng.integers(1 << 30) == b.rng.integers(1 << 30)


@pytest.mark.parametrize("opts", [dict(auto_augment="ra"), dict(auto_augment="ra", ra_num_ops=3, ra_magnitude=4, ta_num_bins=10),
                                  dict(auto_augment="ra", ra_num_ops=1), dict(auto_augment="aa_imagenet")],
                         ids=["ra", "ra-3ops", "ra-1op", "aa_imagenet"])
@pytest.mark.parametrize("kw", MIXES)
def test_new_policies_draw_after_everything_else(kw, opts):
    N, H, W = 8, 32, 64
    a = M.MixSampler(np.random.default_rng(9), N, H, W, **kw)
    b = M.MixSampler(np.random.default_rng(9), N, H, W, **opts, **kw)
    probe = np.random.default_rng(0)
    Kst, bins, mag = opts.get("ra_num_ops", 2), opts.get("ta_num_bins", 31), opts.get("ra_magnitude", 9)
    kinds = set()
    for _ in range(20):
        da, db = a.sample(), b.sample()
        _same_draw(da, db)
        probe.bit_generator.state = a.rng.bit_generator.state  # what b's generator held before the table
        if opts["auto_augment"] == "ra":
            kind, sign = probe.integers(14, size=(Kst, N)), probe.integers(2, size=(Kst, N))
            want = np.stack([np.stack([M.ta_row(int(kind[j, n]), M.ra_magnitude(int(kind[j, n]), mag, int(sign[j, n]),
                                                                                 bins, H, W), H, W)
                                       for n in range(N)]) for j in range(Kst)])
        else:
            Kst = 2
            sub, u, sign = probe.integers(25, size=N), probe.random((2, N)), probe.integers(2, size=(2, N))
            want = np.zeros((2, N, 8), dtype=np.int32)
            for j in range(2):
                for n in range(N):
                    name, prob, b_ = M.AA_IMAGENET[sub[n]][j]
                    k = M.aa_kind(name)
                    m = 0.0 if b_ is None else M.ra_magnitude(k, b_, int(sign[j, n]), 10, H, W)
                    want[j, n] = M.ta_row(k, m, H, W) if u[j, n] <= prob and prob > 0 else M.ta_row(0, 0.0, H, W)
        assert db.ta.shape == (Kst, N, 8) and db.ta.dtype == np.int32 and db["ta"] is db.ta
        assert np.array_equal(db.ta.view(np.float32)[..., 1:], want.view(np.float32)[..., 1:])  # (-0.0 == 0.0)
        assert np.array_equal(db.ta[..., 0], want[..., 0])
        assert probe.bit_generator.state == b.rng.bit_generator.state, "and nothing else is drawn"
        kinds.update(db.ta[..., 0].ravel().tolist())
        a.rng.bit_generator.state = b.rng.bit_generator.state  # keep the two streams aligned for the next step
    assert len(kinds) > 5


# ---------------------------------------------------------------------------------------------
# the fold against Pillow
# ---------------------------------------------------------------------------------------------
NO_ROT = [k for k in range(14) if k != 5]


def _fold(a, rows):
    for row in rows:
        a = R.ta_apply_image(a, row)
    return a


def test_fold_equals_pillow_without_rotate():
    """All 13 x 13 ordered pairs of the kinds other than Rotate, at RandAugment's bin 9 of 31 with either sign, at
    24 x 40: the fold of the definition equals ``transforms.RandAugment.apply`` bit for bit."""
    pytest.importorskip("PIL.Image")
    from dbx_distributed_pytorch_examples_amd.data.transforms import AutoAugment, RandAugment
    H, W = 24, 40
    ims = images(H, W)
    ims = [ims["random"], ims["narrow"], ims["ramp"]]
    for a in NO_ROT:
        for b in NO_ROT:
            for s, im in enumerate(ims):
                rows = M.ra_table([a, b], [9, 9], [s & 1, (s >> 1) & 1], H, W, 31)
                got = np.asarray(RandAugment.apply(im, rows))
                assert np.array_equal(_fold(im, rows), got), (R.TA_NAMES[a], R.TA_NAMES[b], s)
                assert np.array_equal(np.asarray(AutoAugment.apply(im, rows)), got)


def test_fold_with_rotate_is_pinned_stage_by_stage():
    """Brightness -> Rotate -> Equalize: each stage's reference output, computed from the previous stage's
    REFERENCE output, against Pillow applied to that same input. Rotate gets the allowance of
    tests/test_trivial_augment_cpu.py (pixels whose source coordinate lies within 1e-3 of an integer, at most
    2 %), the other stages none."""
    pytest.importorskip("PIL.Image")
    from dbx_distributed_pytorch_examples_amd.data.transforms import RandAugment, TrivialAugmentWide
    H, W = 24, 40
    for s in (0, 1):
        rows = M.ra_table([6, 5, 13], [9, 9, 9], [s, s, s], H, W, 31)
        a = images(H, W)["random"]
        for row in rows:
            got, pil = R.ta_apply_image(a, row), np.asarray(TrivialAugmentWide.apply(a, row))
            if row[0] == 5:
                near = _near_integer(row, H, W)
                assert near.mean() <= 0.02
                assert np.array_equal(got[~near], pil[~near])
            else:
                assert np.array_equal(got, pil)
            a = got
        assert np.asarray(RandAugment.apply(images(H, W)["random"], rows)).shape == (H, W, 3)


def test_cpu_transforms_in_a_compose_chain():
    pytest.importorskip("PIL.Image")
    import random
    from dbx_distributed_pytorch_examples_amd.data.transforms import AutoAugment, Compose, RandAugment
    a = images(24, 40)["random"]
    for t in (RandAugment(), RandAugment(num_ops=3, magnitude=4, num_bins=10), AutoAugment("imagenet")):
        random.seed(3)
        outs = [np.asarray(Compose([t])(a)) for _ in range(40)]
        assert all(o.shape == a.shape and o.dtype == np.uint8 for o in outs)
        assert sum(not np.array_equal(o, a) for o in outs) > 20
    for bad in (dict(num_ops=0), dict(num_ops=5), dict(magnitude=31), dict(magnitude=-1), dict(num_bins=1)):
        with pytest.raises(ValueError):
            RandAugment(**bad)
    with pytest.raises(ValueError):
        AutoAugment("cifar10")


# ---------------------------------------------------------------------------------------------
# the trainer on the CPU path
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts,stages", [(dict(auto_augment="ra"), 2), (dict(auto_augment="aa_imagenet"), 2),
                                         (dict(auto_augment="ra", ra_num_ops=3, ra_magnitude=20), 3)],
                         ids=["ra", "aa_imagenet", "ra-3ops"])
def test_trainer_wiring_on_cpu(opts, stages):
    tr = _trainer(mixup_alpha=0.2, cutmix_alpha=1.0, erase_prob=0.5, erase_mode="pixel", seed=2, **opts)
    p = tr.prog
    N = p.N
    assert p.mix_arena.numel() == (5 + 8 * stages) * N + 6 and not p.ta_ops.any() and p.ta_stages == stages
    assert tuple(p.ta_ops.shape) == (stages, N, 8) and p.ta_work.numel() == K.ta_work_words(N, 32, 32, stages)
    assert tuple(p.ta_T.shape) == (2, N, 32, 32, 4) and tuple(p.ta_hist.shape) == (stages, N, 4, 256)
    img = torch.randint(0, 256, (4, 32, 32, 3), dtype=torch.uint8)
    lab = torch.randint(0, 10, (4,))
    for i in range(4):
        tr.step(img, lab)
        d = tr.last_mix
        assert d["ta"].shape == (stages, N, 8) and p.ta_ops.tolist() == d.ta.tolist()
        want = torch.empty_like(p.x4)
        work = torch.zeros(K.ta_work_words(N, 32, 32, stages), dtype=torch.int32)
        K.chain_augment_u8(p.img_u8, want, p.boxes, p.mean_t.tolist(), p.std_t.tolist(), p.flip, torch.from_numpy(d.ta),
                           work, perm=p.mix_perm, mixbox=p.mix_box, blend=p.mix_blend, erase=p.erase_box,
                           erase_mode="pixel", erase_rng=(p.erase_seed, p.erase_off))
        assert torch.equal(p.x4, want)
    assert tr._mix_ring[0][0].numel() == p.mix_arena.numel(), "a ring slot sized to the arena: one copy per step"
    tr.evaluate_batch(img, lab)
    plain = torch.empty_like(p.x4)
    K.augment_u8(p.img_u8, plain, p.boxes, p.mean_t.tolist(), p.std_t.tolist(), p.flip)
    assert torch.equal(p.x4, plain), "evaluation never augments"
    s = tr.mix_summary()
    assert s["auto_augment"] == opts["auto_augment"] and s["kernel"] == "chain_augment_u8" and s["num_ops"] == stages
    assert s["magnitude"] == (opts.get("ra_magnitude", 9) if opts["auto_augment"] == "ra" else None)


def test_earlier_policies_allocate_what_they_allocated():
    ta = _trainer(auto_augment="ta_wide", seed=1).prog
    assert ta.ta_work.numel() == K.ta_work_words(4, 32, 32) and tuple(ta.ta_ops.shape) == (4, 8)
    assert tuple(ta.ta_T.shape) == (4, 32, 32, 4) and ta.mix_arena.numel() == 13 * 4 + 6 and ta.ta_stages == 1
    off = _trainer(seed=1).prog
    assert off.ta_work is None and off.ta_ops is None and off.mix_arena is None and off.ta_stages == 0
    one = _trainer(auto_augment="ra", ra_num_ops=1, seed=1)
    assert one.prog.ta_work.numel() == K.ta_work_words(4, 32, 32) and one.mix_summary()["kernel"] == "trivial_augment_u8"


# ---------------------------------------------------------------------------------------------
# config and refusals
# ---------------------------------------------------------------------------------------------
BAD = [dict(auto_augment="ra", ra_num_ops=0), dict(auto_augment="ra", ra_num_ops=5), dict(auto_augment="ra", ra_num_ops=2.0),
       dict(auto_augment="ra", ra_magnitude=31), dict(auto_augment="ra", ra_magnitude=-1),
       dict(auto_augment="ra", ra_magnitude=9, ta_num_bins=9), dict(auto_augment="ra", ta_num_bins=1),
       dict(ra_num_ops=3), dict(ra_magnitude=5), dict(auto_augment="ta_wide", ra_num_ops=3),
       dict(auto_augment="aa_imagenet", ra_magnitude=5), dict(auto_augment="aa_cifar10"), dict(auto_augment="randaugment")]


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_bad_values_raise(kw, monkeypatch):
    from dbx_distributed_pytorch_examples_amd import config as C
    from dbx_distributed_pytorch_examples_amd.train import engine as E
    with pytest.raises(ValueError):
        M.validate_auto_augment(**kw)
    with pytest.raises(ValueError):
        M.MixSampler(np.random.default_rng(0), 4, 32, 32, **kw)
    with pytest.raises(ValueError):
        _trainer(**kw)
    cfg = C.TrainConfig(model="resnet18", num_classes=10, batch_size=4, max_steps=1)
    cfg.data.image_size, cfg.data.train_samples = 32, 8
    for k, v in kw.items():
        setattr(cfg.data, k, v)
    with pytest.raises(ValueError):
        C.validate_data(cfg.data)
    with pytest.raises(ValueError):
        C.auto_augment_options(cfg.data)
    monkeypatch.setenv("DBX_FORCE_CPU", "1")
    monkeypatch.setattr(E, "_Autograd", lambda *a, **k: (_ for _ in ()).throw(AssertionError("built a runner")))
    with pytest.raises(ValueError):
        E.train(cfg, log_mlflow=False)


@pytest.mark.parametrize("policy", ["ra", "aa_imagenet"])
def test_trainers_and_train_refuse_what_they_cannot_do(policy, monkeypatch):
    from dbx_distributed_pytorch_examples_amd import config as C
    from dbx_distributed_pytorch_examples_amd.engine.autograd_trainer import AutogradTrainer
    from dbx_distributed_pytorch_examples_amd.engine.frozen_trainer import FrozenFeatureTrainer
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import OptimConfig
    from dbx_distributed_pytorch_examples_amd.engine.program import ResNetProgram
    from dbx_distributed_pytorch_examples_amd.models import FrozenBackboneClassifier, build_model
    from dbx_distributed_pytorch_examples_amd.train import engine as E
    with pytest.raises(ValueError, match="auto_augment"):
        AutogradTrainer(build_model("resnet18", num_classes=10), CPU, OptimConfig(), auto_augment=policy)
    with pytest.raises(ValueError, match="auto_augment"):
        FrozenFeatureTrainer(FrozenBackboneClassifier("resnet18", num_classes=10), 4, (32, 32), CPU, OptimConfig(),
                             auto_augment=policy)
    gray = build_model("resnet18", num_classes=10, in_channels=1)
    with pytest.raises(ValueError, match="3-channel"):
        _trainer(gray, auto_augment=policy)
    with pytest.raises(ValueError, match="3-channel"):
        ResNetProgram(gray, 4, (32, 32), CPU).enable_mix(ta=2)
    with pytest.raises(ValueError, match="0..4"):
        ResNetProgram(build_model("resnet18", num_classes=10), 4, (32, 32), CPU).enable_mix(ta=5)

    monkeypatch.setenv("DBX_FORCE_CPU", "1")
    boom = lambda *a, **k: (_ for _ in ()).throw(AssertionError("built a runner"))  # noqa: E731
    monkeypatch.setattr(E, "_Autograd", boom)
    monkeypatch.setattr(E, "_Native", boom)

    def cfg(**kw):
        c = C.TrainConfig(model="resnet18", num_classes=10, batch_size=4, max_steps=1, **kw)
        c.data.image_size, c.data.train_samples, c.data.auto_augment = 32, 8, policy
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
    cfg = C.load_config(overrides=["data.auto_augment=ra", "data.ra_num_ops=3", "data.ra_magnitude=4", "data.ta_num_bins=11"])
    assert C.auto_augment_options(cfg.data) == dict(auto_augment="ra", ta_num_bins=11, ra_num_ops=3, ra_magnitude=4)
    aa = C.load_config(overrides=["data.auto_augment=aa_imagenet"])
    assert C.auto_augment_options(aa.data) == dict(auto_augment="aa_imagenet", ta_num_bins=31)
    d = C.TrainConfig().data
    assert (d.ra_num_ops, d.ra_magnitude) == M.RA_DEFAULTS == (2, 9)
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs")
    ra = C.load_config(os.path.join(root, "resnet50_imagenet_8192_recipe_ra.yaml"))
    base = C.load_config(os.path.join(root, "resnet50_imagenet_8192_recipe.yaml"))
    assert (ra.data.auto_augment, ra.data.ra_num_ops, ra.data.ra_magnitude, ra.data.ta_num_bins) == ("ra", 2, 9, 31)
    C.validate_data(ra.data)
    tr = _trainer(**C.auto_augment_options(ra.data))
    assert tr.mix_summary()["kernel"] == "chain_augment_u8" and tr.prog.ta_stages == 2
    ra.data.auto_augment = None
    assert C.to_dict(ra) == C.to_dict(base), "the recipe config plus the one option"
    with pytest.raises(ValueError):
        C.validate_data(C.load_config(overrides=["data.ra_num_ops=3"]).data)
    with pytest.raises(ValueError):
        C.validate_data(C.load_config(os.path.join(root, "resnet50_imagenet_8192_recipe_ra.yaml"),
                                      overrides=["data.ra_magnitude=31"]).data)
