"""The resampling filters' definition (ops/reference.py) against Pillow, the relation between the filters, and what
needs no GPU: the config fields and the refusals."""
import os

import numpy as np
import pytest
import torch

from dbx_distributed_pytorch_examples_amd import config as C
from dbx_distributed_pytorch_examples_amd.ops import kernels as K
from dbx_distributed_pytorch_examples_amd.ops import reference as R

CPU = torch.device("cpu")
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
# (H, W, Ho, Wo, box = (y0, x0, h, w) or None for the whole image): up- and down-scaling, fractional boxes, 1 x 1
SHAPES = [(37, 53, 8, 8, None), (20, 20, 16, 16, (3.25, 2.5, 6.5, 7.75)), (5, 640, 3, 300, None),
          (3, 1400, 4, 100, None), (1, 1, 4, 4, None), (48, 64, 32, 32, (0.3, 0.6, 38.5, 57.6)), (23, 31, 19, 9, None)]


def _case(shape, lo=0, hi=256):
    H, W, Ho, Wo, box = shape
    img = torch.from_numpy(np.random.default_rng(H * W).integers(lo, hi, (1, H, W, 3), dtype=np.uint8))
    return img, torch.tensor([box or (0.0, 0.0, H, W)], dtype=torch.float32)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("name", ["aa_bilinear", "aa_bicubic"])
def test_definition_against_pillow(name, shape):
    """Pillow rounds to uint8 after its horizontal pass and at the end, with 22-bit coefficients; for bicubic it also
    clips that intermediate, so those sources stay in [64, 192], where the horizontal pass cannot leave 0..255."""
    from PIL import Image
    H, W, Ho, Wo, _ = shape
    img, boxes = _case(shape, *((64, 193) if name == "aa_bicubic" else (0, 256)))
    y0, x0, h, w = boxes[0].tolist()
    pil = Image.fromarray(img[0].numpy()).resize(
        (Wo, Ho), Image.BICUBIC if name == "aa_bicubic" else Image.BILINEAR, box=(x0, y0, x0 + w, y0 + h))
    (v, _), = R.resample_v64(img, Ho, Wo, boxes, None, name)
    My, _ = R.resample_axis(y0, h, Ho, H, name)
    bound = 0.5 * np.abs(My).sum(1)[:, None, None] + 0.5 + 0.01
    err = np.abs(np.asarray(pil).astype(np.float64) - v)
    print(f"{name} {shape}: largest err / bound {(err / bound).max():.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[4]], ids=str)
def test_bicubic_is_the_antialiased_filter_where_nothing_shrinks(shape):
    H, W, Ho, Wo, _ = shape
    img, boxes = _case(shape)
    (a, _), = R.resample_v64(img, Ho, Wo, boxes, None, "bicubic")
    (b, _), = R.resample_v64(img, Ho, Wo, boxes, None, "aa_bicubic")
    assert np.array_equal(a, b)


def test_cpu_path_and_the_wrappers_refusals():
    img, boxes = _case(SHAPES[5])
    out = torch.zeros(1, 32, 32, 4, dtype=torch.bfloat16)
    K.augment_u8(img, out, boxes, MEAN, STD, resample="aa_bicubic")
    work = torch.zeros(K.ta_work_words(1, 32, 32), dtype=torch.int32)
    via_t = torch.zeros_like(out)
    K.trivial_augment_u8(img, via_t, boxes, MEAN, STD, None, torch.zeros(1, 8, dtype=torch.int32), work,
                         resample="aa_bicubic")
    assert torch.equal(out, via_t)
    T, hist, _, _ = K.ta_work_views(work, 1, 32, 32)
    perm, box = torch.zeros(1, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    for kw in (dict(perm=perm, mixbox=box), dict(erase=torch.zeros(1, 4, dtype=torch.int32)),
               dict(perm=perm, blend=torch.ones(1))):
        with pytest.raises(ValueError, match="trivial_augment_u8"):
            K.augment_u8(img, out, boxes, MEAN, STD, resample="bicubic", **kw)
    for fn in (lambda: K.augment_u8(img, out, boxes, MEAN, STD, resample="lanczos"),
               lambda: K.crop_resize_u8(img, T, hist, boxes, resample="bilinear"),
               lambda: K.trivial_augment_u8(img, out, boxes, MEAN, STD, None, None, work, resample=3)):
        with pytest.raises(ValueError, match="resample must be"):
            fn()


def test_config_fields_and_the_engines_that_refuse_them(monkeypatch):
    from dbx_distributed_pytorch_examples_amd.data.datasets import SyntheticImages
    from dbx_distributed_pytorch_examples_amd.engine.autograd_trainer import AutogradTrainer
    from dbx_distributed_pytorch_examples_amd.engine.frozen_trainer import FrozenFeatureTrainer
    from dbx_distributed_pytorch_examples_amd.engine.native_module import native_module
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer
    from dbx_distributed_pytorch_examples_amd.models import FrozenBackboneClassifier, build_model
    from dbx_distributed_pytorch_examples_amd.train import engine as E
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = C.load_config(os.path.join(root, "configs", "resnet50_imagenet_8192_a2_ragged.yaml"))
    assert cfg.data.resample == "aa_bicubic" and cfg.data.eval_resample is None and cfg.data.ragged
    C.validate_train(cfg)
    for bad in (dict(resample="lanczos"), dict(eval_resample=2)):
        with pytest.raises(ValueError, match="resample"):
            C.validate_data(C.DataConfig(**bad))
    o = C.OptimizerConfig()
    for kw in (dict(resample="bicubic"), dict(eval_resample="aa_bilinear")):
        with pytest.raises(ValueError, match="resample"):
            AutogradTrainer(build_model("resnet18", num_classes=10), CPU, o, **kw)
        with pytest.raises(ValueError, match="resample"):
            FrozenFeatureTrainer(FrozenBackboneClassifier("resnet18", num_classes=10), 4, (32, 32), CPU, o, **kw)
        with pytest.raises(ValueError, match="resample"):
            native_module(build_model("resnet18", num_classes=10), 4, (32, 32), CPU, **kw)
    with pytest.raises(ValueError, match="resample must be"):
        NativeTrainer(build_model("resnet18", num_classes=10), 4, (32, 32), CPU, resample="nearest")
    monkeypatch.setenv("DBX_FORCE_CPU", "1")
    cfg = C.TrainConfig(model="resnet18", num_classes=10, batch_size=4, engine="autograd")
    cfg.data.image_size, cfg.data.resample = 32, "aa_bicubic"
    with pytest.raises(ValueError, match="autograd engine"):
        E.train(cfg, train_dataset=SyntheticImages(8, 32, 3, 10), log_mlflow=False)
    cfg.engine = "native"
    with pytest.raises(ValueError, match="frozen-backbone"):
        E.train(cfg, model=FrozenBackboneClassifier("resnet18", num_classes=10),
                train_dataset=SyntheticImages(8, 32, 3, 10), log_mlflow=False)
