"""The resampling filter in the native step (ResNet-18, batch 16, 32x32, ragged): its input is the standalone call."""
import copy

import pytest
import torch

from dbx_distributed_pytorch_examples_amd.engine.program import ResNetProgram
from dbx_distributed_pytorch_examples_amd.ops import kernels as K
from test_ragged_trainer_gpu import HW, MAX_HW, N, dev, models, norm, ragged_batches, trainer

pytestmark = pytest.mark.gpu
MIX = dict(mixup_alpha=0.2, cutmix_alpha=1.0, erase_prob=0.5, erase_mode="pixel")


@pytest.mark.parametrize("opts", [dict(), MIX], ids=["plain", "mixup-cutmix-erase"])
def test_step_input_is_the_standalone_call(opts):
    # six steps (two eager warm-ups, the capture, three replays), a different packing each
    m1, m2 = models()
    a = trainer(m1, src_ragged=MAX_HW, seed=4, use_graphs=True, resample="aa_bicubic", **opts)
    b = trainer(m2, src_ragged=MAX_HW, seed=4, use_graphs=False, resample="aa_bicubic", **opts)
    for i, ((packed, lab, boxes, flips, table), _) in enumerate(ragged_batches(6, seed=2)):
        p = a.prog
        a.step(packed, lab, boxes, flips, src_table=table)
        b.step(packed, lab, boxes, flips, src_table=table)
        assert torch.equal(p.x4, b.prog.x4) and torch.equal(p.master, b.prog.master), i
        want = torch.full_like(p.x4, float("nan"))
        if opts:  # paste, blend and erase on the filtered uint8 batch: the pipeline with an Identity table
            T, hist, lut, tmean = K.ta_work_views(torch.zeros_like(p.rs_work), N, HW, HW)
            K.crop_resize_u8(p.img_u8, T, hist, p.boxes, p.flip, src=p.src_tab, resample="aa_bicubic")
            K.ta_prepare(hist, p.rs_ops, lut, tmean)
            K.ta_apply_u8(T, want, p.rs_ops, lut, tmean, *norm(p), perm=p.mix_perm, mixbox=p.mix_box, blend=p.mix_blend,
                          erase=p.erase_box, erase_mode="pixel", erase_rng=(p.erase_seed, p.erase_off.clone()))
        else:
            K.augment_u8(p.img_u8, want, p.boxes, *norm(p), p.flip, src=p.src_tab, resample="aa_bicubic")
        assert torch.equal(p.x4, want), i
    assert a.graphs and not b.graphs


def test_eval_uses_eval_resample_and_never_augments():
    m1, _ = models()
    a = trainer(m1, src_ragged=MAX_HW, seed=6, resample="aa_bicubic", eval_resample="aa_bilinear", **MIX)
    same = ResNetProgram(copy.deepcopy(m1), N, (HW, HW), dev(), resample="bicubic")
    assert (a.prog.resample, a.prog.eval_resample, same.eval_resample) == ("aa_bicubic", "aa_bilinear", "bicubic")
    for (packed, lab, boxes, flips, table), _ in ragged_batches(2, seed=5):
        a.step(packed, lab, boxes, flips, src_table=table)
    p = a.prog
    a.eval_begin()
    for i in range(4):  # two eager calls, the capture, a replay
        (packed, lab, boxes, _, table), _ = ragged_batches(1, seed=20 + i)[0]
        a.eval_step(packed, lab, boxes, src_table=table)
        want = torch.full_like(p.x4, float("nan"))
        K.augment_u8(p.img_u8, want, p.boxes, *norm(p), p.flip, src=p.src_tab, resample="aa_bilinear")
        assert torch.equal(p.x4, want), i
    assert a.eval_end().count == 4 * N


def test_refusals():
    m1, _ = models()
    with pytest.raises(ValueError, match="resample must be"):
        trainer(m1, resample="lanczos")
    gray = copy.deepcopy(m1)
    gray.conv1 = torch.nn.Conv2d(1, 64, 3, 1, 1, bias=False)
    with pytest.raises(ValueError, match="3-channel"):
        trainer(gray, resample="bicubic", erase_prob=0.5)
    with pytest.raises(ValueError, match="3-channel"):
        ResNetProgram(gray, N, (HW, HW), dev(), resample="bicubic").enable_cutmix()
    assert trainer(m1, cutmix_alpha=1.0).prog.rs_work is None  # (no filter: nothing more is allocated)
