"""The host side of batch mixing (engine/mix.py) and everything above the kernel that runs without a GPU:
the per-step sampler, the erase boxes, the unchanged CutMix-only draw sequence of the native trainer, the
config checks, engine selection, the autograd engine's torch versions and the Composer frontend."""
import math

import numpy as np
import pytest
import torch

from dbx_distributed_pytorch_examples_amd.engine.mix import MixSampler, sample_erase_boxes, validate_mix

CPU = torch.device("cpu")
STEPS = 2000


def _sigma(p, n):
    return math.sqrt(p * (1 - p) / n)


# ---------------------------------------------------------------------------------------------
# the sampler
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mix_prob,switch", [(1.0, 0.5), (0.7, 0.3)])
def test_sampler_kinds_and_weights(mix_prob, switch):
    N, H, W = 8, 32, 32
    s = MixSampler(np.random.default_rng(11), N, H, W, mixup_alpha=0.2, cutmix_alpha=1.0, mix_prob=mix_prob,
                   mix_switch_prob=switch, erase_prob=0.25)
    kinds = {"none": 0, "mixup": 0, "cutmix": 0}
    for _ in range(STEPS):
        d = s.sample()
        kinds[d.kind] += 1
        y0, y1, x0, x1 = d.box
        area = max(y1 - y0, 0) * max(x1 - x0, 0)
        assert not (d.blend < 1.0 and area > 0), "MixUp and CutMix are never both applied in one step"
        assert sorted(d.perm.tolist()) == list(range(N)) and d.perm.dtype == np.int32
        assert d.erase.shape == (N, 4) and d.erase.dtype == np.int32
        if d.kind == "none":
            assert d.blend == 1.0 and d.lam == 1.0 and area == 0 and d.perm.tolist() == list(range(N))
        elif d.kind == "mixup":
            assert d.lam == d.blend and 0.0 <= d.lam <= 1.0 and area == 0
            assert d.lam == float(np.float32(d.lam)), "one fp32 number for the blend and the CE weight"
        else:
            assert d.blend == 1.0 and 0 <= y0 <= y1 <= H and 0 <= x0 <= x1 <= W
            assert d.lam == 1.0 - area / (H * W)
    mixed = kinds["mixup"] + kinds["cutmix"]
    assert abs(kinds["none"] / STEPS - (1 - mix_prob)) <= 5 * _sigma(1 - mix_prob, STEPS) + 1e-12
    assert abs(kinds["cutmix"] / mixed - switch) <= 5 * _sigma(switch, mixed)


@pytest.mark.parametrize("alphas,kind", [((0.2, 0.0), "mixup"), ((0.0, 1.0), "cutmix"), ((0.0, 0.0), "none")])
def test_sampler_with_one_alpha_takes_that_one(alphas, kind):
    s = MixSampler(np.random.default_rng(3), 4, 16, 16, mixup_alpha=alphas[0], cutmix_alpha=alphas[1], erase_prob=0.5)
    assert {s.sample().kind for _ in range(50)} == {kind}


# ---------------------------------------------------------------------------------------------
# erase boxes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [32, 224])
@pytest.mark.parametrize("scale,ratio", [((0.02, 1 / 3), (0.3, 3.3)), ((0.1, 0.2), (0.5, 2.0))])
def test_erase_boxes(hw, scale, ratio):
    H = W = hw
    n = 4000
    b = sample_erase_boxes(np.random.default_rng(5), n, H, W, 0.25, scale, ratio)
    assert b.shape == (n, 4) and b.dtype == np.int32
    h, w = (b[:, 1] - b[:, 0]).astype(np.float64), (b[:, 3] - b[:, 2]).astype(np.float64)
    on = (h > 0) | (w > 0)
    assert bool((b[~on] == 0).all())
    assert abs(on.mean() - 0.25) <= 5 * _sigma(0.25, n)  # (a no-fit is far rarer than this at these ranges)
    b, h, w = b[on], h[on], w[on]
    assert bool(((b[:, 0] >= 0) & (b[:, 1] <= H) & (b[:, 2] >= 0) & (b[:, 3] <= W)).all()), "inside the image"
    assert bool(((h >= 1) & (h < H) & (w >= 1) & (w < W)).all())
    # h = round(sqrt(area ar)), w = round(sqrt(area / ar)): the unrounded sides lie within 1/2 of them
    assert bool(((h + 0.5) * (w + 0.5) >= scale[0] * H * W).all()) and bool(((h - 0.5) * (w - 0.5) <= scale[1] * H * W).all())
    assert bool(((h + 0.5) / (w - 0.5) >= ratio[0]).all()) and bool(((h - 0.5) / (w + 0.5) <= ratio[1]).all())
    # positions are spread over the whole admissible range
    assert b[:, 0].min() == 0 and b[:, 2].min() == 0 and b[:, 1].max() == H and b[:, 3].max() == W


def test_erase_prob_extremes():
    rng = np.random.default_rng(6)
    assert not sample_erase_boxes(rng, 500, 32, 32, 0.0).any()
    b = sample_erase_boxes(rng, 500, 32, 32, 1.0)
    assert bool(((b[:, 1] > b[:, 0]) & (b[:, 3] > b[:, 2])).all())
    # ratios that fit only sometimes (h = 4 w with area >= 0.9 H W needs h >= 61 > H): a valid box or an empty one
    b = sample_erase_boxes(rng, 500, 32, 32, 1.0, scale=(0.2, 1.0), ratio=(3.0, 4.0))
    h, w = b[:, 1] - b[:, 0], b[:, 3] - b[:, 2]
    empty = (b == 0).all(axis=1)
    assert empty.any() and not empty.all()
    assert bool(((h >= 1) & (h < 32) & (w >= 1) & (w < 32))[~empty].all())
    # no try can fit: every sample stays un-erased
    assert not sample_erase_boxes(rng, 50, 8, 8, 1.0, scale=(0.99, 1.0), ratio=(1.0, 1.0)).any()


# ---------------------------------------------------------------------------------------------
# the CutMix-only sequence of the native trainer is the one it has always drawn
# ---------------------------------------------------------------------------------------------
def _trainer(**kw):
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer
    from dbx_distributed_pytorch_examples_amd.models import build_model
    torch.manual_seed(0)
    return NativeTrainer(build_model("resnet18", num_classes=10), 4, (32, 32), CPU, **kw)


def test_cutmix_only_sequence_unchanged():
    seed, N, H, W = 5, 4, 32, 32
    tr = _trainer(cutmix_alpha=1.0, seed=seed)
    assert tr.prog.mix_blend is None and tr.prog.erase_box is None, "CutMix alone allocates nothing new"
    img = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8)
    lab = torch.randint(0, 10, (N,))
    r = np.random.default_rng(seed)
    for _ in range(5):
        tr.step(img, lab)
        # the documented rule: beta, integers, integers, permutation
        lam = float(r.beta(1.0, 1.0))
        cut = (1.0 - lam) ** 0.5
        ch, cw = int(H * cut), int(W * cut)
        cy, cx = int(r.integers(0, H)), int(r.integers(0, W))
        y0, y1 = min(max(cy - ch // 2, 0), H), min(max(cy + ch // 2, 0), H)
        x0, x1 = min(max(cx - cw // 2, 0), W), min(max(cx + cw // 2, 0), W)
        lam = 1.0 - (y1 - y0) * (x1 - x0) / float(H * W)
        perm = r.permutation(N).astype("int32")
        d = tr.last_mix
        assert d.kind == "cutmix" and d.box == (y0, y1, x0, x1) and d.lam == lam and d.erase is None
        assert d.perm.tolist() == perm.tolist()
        assert tr.prog.mix_perm.tolist() == perm.tolist() and tr.prog.mix_box.tolist() == [y0, y1, x0, x1]
        assert float(tr.prog.mix_lam) == float(np.float32(lam))


def test_trainer_all_options_on_cpu():
    """The program's tables follow the host draw, the Philox offset advances by one per step, evaluation
    never mixes or erases, and the summary names the settings."""
    from dbx_distributed_pytorch_examples_amd.ops import kernels as K
    tr = _trainer(mixup_alpha=0.2, cutmix_alpha=1.0, erase_prob=0.5, erase_mode="pixel", seed=2)
    p = tr.prog
    assert float(p.mix_blend) == 1.0 and not p.erase_box.any() and int(p.erase_off) == 0
    img = torch.randint(0, 256, (4, 32, 32, 3), dtype=torch.uint8)
    lab = torch.randint(0, 10, (4,))
    kinds = set()
    for i in range(6):
        tr.step(img, lab)
        d = tr.last_mix
        kinds.add(d.kind)
        assert int(p.erase_off) == i + 1
        assert float(p.mix_blend) == d.blend and float(p.mix_lam) == float(np.float32(d.lam))
        assert p.erase_box.tolist() == d.erase.tolist() and p.mix_perm.tolist() == d.perm.tolist()
        want = torch.empty_like(p.x4)
        K.augment_u8(p.img_u8, want, p.boxes, p.mean_t.tolist(), p.std_t.tolist(), p.flip, perm=p.mix_perm,
                     mixbox=p.mix_box, blend=p.mix_blend, erase=p.erase_box, erase_mode="pixel",
                     erase_rng=(p.erase_seed, p.erase_off))
        assert torch.equal(p.x4, want)
    assert len(kinds) == 2
    tr.evaluate_batch(img, lab)
    plain = torch.empty_like(p.x4)
    K.augment_u8(p.img_u8, plain, p.boxes, p.mean_t.tolist(), p.std_t.tolist(), p.flip)
    assert torch.equal(p.x4, plain) and int(p.erase_off) == 6
    s = tr.mix_summary()
    assert s["mixup_alpha"] == 0.2 and s["erase_mode"] == "pixel" and s["kernel"] == "augment_mix_u8"


def test_options_off_allocate_nothing():
    tr = _trainer(mixup_alpha=0.0, erase_prob=0.0)
    assert tr.prog.mix_blend is None and tr.prog.mix_perm is None and tr.last_mix is None and not tr.prog.cutmix
    assert tr.mix_summary()["kernel"] == "augment_u8"


# ---------------------------------------------------------------------------------------------
# config, engine selection, autograd engine, frontend
# ---------------------------------------------------------------------------------------------
BAD = [dict(mixup_alpha=-0.1), dict(cutmix_alpha=-1.0), dict(mixup_alpha=float("nan")), dict(mix_prob=1.5),
       dict(mix_switch_prob=-0.1), dict(erase_prob=2.0), dict(erase_mode="noise"), dict(erase_scale=(0.5, 0.1)),
       dict(erase_scale=(0.0, 0.3)), dict(erase_scale=(0.1, 1.5)), dict(erase_ratio=(3.0, 0.3)),
       dict(erase_ratio=(0.0, 1.0)), dict(erase_ratio=(1.0,))]


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_bad_values_raise(kw, monkeypatch):
    from dbx_distributed_pytorch_examples_amd import config as C
    from dbx_distributed_pytorch_examples_amd.train import engine as E
    with pytest.raises(ValueError):
        validate_mix(**kw)
    cfg = C.TrainConfig(model="resnet18", num_classes=10, batch_size=4, max_steps=1)
    cfg.data.image_size, cfg.data.train_samples = 32, 8
    for k, v in kw.items():
        setattr(cfg.data, k, v)
    with pytest.raises(ValueError):
        C.mix_options(cfg.data)
    monkeypatch.setenv("DBX_FORCE_CPU", "1")
    monkeypatch.setattr(E, "_Autograd", lambda *a, **k: (_ for _ in ()).throw(AssertionError("built a runner")))
    with pytest.raises(ValueError):
        E.train(cfg, log_mlflow=False)


def test_config_loads_and_reaches_the_trainers():
    from dbx_distributed_pytorch_examples_amd import config as C
    cfg = C.load_config(overrides=["data.mixup_alpha=0.2", "data.erase_prob=0.1", "data.erase_mode=pixel",
                                   "data.erase_scale=[0.05, 0.2]", "data.mix_switch_prob=0.25"])
    kw = C.mix_options(cfg.data)
    assert kw == dict(mixup_alpha=0.2, cutmix_alpha=0.0, mix_prob=1.0, mix_switch_prob=0.25, erase_prob=0.1,
                      erase_mode="pixel", erase_scale=(0.05, 0.2), erase_ratio=(0.3, 3.3))
    import os
    recipe = C.load_config(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs",
                                        "resnet50_imagenet_8192_recipe.yaml"))
    d = recipe.data
    assert (d.label_smoothing, d.mixup_alpha, d.cutmix_alpha, d.erase_prob) == (0.1, 0.2, 1.0, 0.1)
    assert recipe.ema_decay > 0 and recipe.optim.norm_weight_decay == 0 and recipe.optim.bias_weight_decay == 0
    C.mix_options(d)


@pytest.mark.parametrize("opt", [dict(cutmix_alpha=1.0), dict(mixup_alpha=0.2), dict(erase_prob=0.1)])
def test_pick_engine_routes_frozen_backbone_to_autograd(opt):
    from dbx_distributed_pytorch_examples_amd.config import TrainConfig
    from dbx_distributed_pytorch_examples_amd.data.datasets import SyntheticImages
    from dbx_distributed_pytorch_examples_amd.models import FrozenBackboneClassifier, build_model
    from dbx_distributed_pytorch_examples_amd.train.engine import _pick_engine
    ds, cuda = SyntheticImages(8, 32, 3, 10), torch.device("cuda")
    cfg = TrainConfig(model="resnet18", num_classes=10, batch_size=4)
    frozen = FrozenBackboneClassifier("resnet18", num_classes=10)
    assert _pick_engine(cfg, frozen, ds, cuda) == "native"
    for k, v in opt.items():
        setattr(cfg.data, k, v)
    assert _pick_engine(cfg, frozen, ds, cuda) == "autograd"
    assert _pick_engine(cfg, build_model("resnet18", num_classes=10), ds, cuda) == "native"


def test_autograd_mixup_definition():
    from dbx_distributed_pytorch_examples_amd.engine.autograd_trainer import mixup
    g = torch.Generator().manual_seed(4)
    x, y = torch.randn(8, 3, 16, 16, generator=g), torch.arange(8)
    out, tgt = mixup(x, y, 8, 0.2, g)
    lam = float(tgt[0, 0])
    assert 0.0 < lam < 1.0 and lam != 0.5
    rest = tgt.clone()
    rest[torch.arange(8), y] = 0.0
    perm = rest.argmax(1)
    fixed = rest.sum(1) == 0  # (a fixed point of the permutation keeps its whole weight)
    perm[fixed] = y[fixed]
    assert sorted(perm.tolist()) == list(range(8))
    want_t = lam * torch.eye(8) + (1 - lam) * torch.eye(8)[perm]
    assert torch.allclose(tgt, want_t, atol=1e-6) and torch.allclose(tgt.sum(1), torch.ones(8), atol=1e-6)
    assert torch.allclose(out, lam * x + (1 - lam) * x[perm], atol=1e-6)
    same, t1 = mixup(x, y, 8, 0.0, g)  # alpha 0: lam = 1
    assert torch.equal(same, x) and torch.equal(t1, torch.eye(8))


@pytest.mark.parametrize("mode", ["const", "pixel"])
def test_autograd_random_erase_definition(mode):
    from dbx_distributed_pytorch_examples_amd.engine.autograd_trainer import random_erase
    g = torch.Generator().manual_seed(9)
    x = torch.randn(8, 3, 16, 16, generator=g) + 3.0  # (no element is 0)
    scale, ratio = (0.02, 1 / 3), (0.3, 3.3)
    assert random_erase(x, 0.0, scale, ratio, mode, g) is x
    hit = 0
    for _ in range(20):
        out = random_erase(x, 0.5, scale, ratio, mode, g)
        for i in range(8):
            ch = (out[i] != x[i]).any(0)
            if not ch.any():
                continue
            hit += 1
            ys, xs = ch.any(1).nonzero().flatten(), ch.any(0).nonzero().flatten()
            y0, y1, x0, x1 = int(ys[0]), int(ys[-1]) + 1, int(xs[0]), int(xs[-1]) + 1
            h, w = y1 - y0, x1 - x0
            assert bool(ch[y0:y1, x0:x1].all()) and int(ch.sum()) == h * w, "one full rectangle, all channels"
            assert bool((out[i] != x[i])[:, y0:y1, x0:x1].all())
            assert 1 <= h < 16 and 1 <= w < 16
            assert (h + 0.5) * (w + 0.5) >= scale[0] * 256 and (h - 0.5) * (w - 0.5) <= scale[1] * 256
            assert (h + 0.5) / (w - 0.5) >= ratio[0] and (h - 0.5) / (w + 0.5) <= ratio[1]
            if mode == "const":
                assert bool((out[i, :, y0:y1, x0:x1] == 0).all())
    assert 40 <= hit <= 120  # 160 samples at p = 0.5
    full = random_erase(x, 1.0, scale, ratio, mode, g)
    assert all(bool((full[i] != x[i]).any()) for i in range(8))
    with pytest.raises(ValueError):
        random_erase(x, 0.5, scale, ratio, "noise", g)
    if mode == "pixel":
        z = torch.cat([(o := random_erase(x, 1.0, (0.3, 1 / 3), (1.0, 1.0), mode, g))[o != x] for _ in range(40)])
        assert abs(float(z.mean())) < 0.1 and abs(float(z.var()) - 1) < 0.1  # N(0, 1), > 10,000 values


def test_autograd_trainer_applies_the_switch_rule(monkeypatch):
    from dbx_distributed_pytorch_examples_amd.config import OptimizerConfig
    from dbx_distributed_pytorch_examples_amd.engine import autograd_trainer as A
    from dbx_distributed_pytorch_examples_amd.models import build_model
    torch.manual_seed(1)
    calls = []
    for name in ("cutmix", "mixup"):
        real = getattr(A, name)
        monkeypatch.setattr(A, name, lambda *a, _n=name, _r=real, **k: (calls.append(_n), _r(*a, **k))[1])
    real_er = A.random_erase
    monkeypatch.setattr(A, "random_erase", lambda *a, **k: (calls.append("erase"), real_er(*a, **k))[1])
    tr = A.AutogradTrainer(build_model("resnet18", num_classes=10), CPU, OptimizerConfig(name="sgd", lr=0.01),
                           cutmix_alpha=1.0, mixup_alpha=0.2, mix_prob=0.8, mix_switch_prob=0.5, erase_prob=0.25)
    x, y = torch.randn(4, 3, 32, 32), torch.randint(0, 10, (4,))
    kinds = [tr._mix_kind() for _ in range(400)]
    assert abs(kinds.count("none") / 400 - 0.2) <= 5 * _sigma(0.2, 400)
    mixed = 400 - kinds.count("none")
    assert abs(kinds.count("cutmix") / mixed - 0.5) <= 5 * _sigma(0.5, mixed)
    for _ in range(4):
        n0 = len(calls)
        tr.step(x, y)
        got = calls[n0:]
        assert got[0] == "erase" and len(got) <= 2 and set(got[1:]) <= {"cutmix", "mixup"}  # erase first, one mix
    with pytest.raises(ValueError):
        A.AutogradTrainer(build_model("resnet18", num_classes=10), CPU, OptimizerConfig(), mixup_alpha=-1.0)


def test_composer_mixup_is_picked_up():
    from dbx_distributed_pytorch_examples_amd.frontends.composer import CutMix, LabelSmoothing, MixUp, Trainer
    from dbx_distributed_pytorch_examples_amd.models import build_model
    assert MixUp().alpha == 0.2
    t = Trainer(build_model("resnet18", num_classes=10), algorithms=[LabelSmoothing(0.1), MixUp(0.4)], device="cpu")
    assert t.tr.mixup_alpha == 0.4 and t.tr.cutmix_alpha == 0.0 and t.tr.smoothing == 0.1
    t = Trainer(build_model("resnet18", num_classes=10), algorithms=[CutMix(1.0), MixUp(num_classes=10)], device="cpu")
    assert t.tr.mixup_alpha == 0.2 and t.tr.cutmix_alpha == 1.0 and t.tr.num_classes == 10
