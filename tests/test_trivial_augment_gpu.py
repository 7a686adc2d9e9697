"""TrivialAugmentWide inside the native training step, on the GPU: ResNet-18, 10 classes, batch 8, 32x32,
4 steps (two eager warm-ups, the capture, one replay). What the captured step feeds the network is the
pipeline's output for the table the host sampled; a replayed graph follows the table; evaluation never
augments; with the option off nothing changes."""
import copy

import pytest
import torch

from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig
from dbx_distributed_pytorch_examples_amd.models import build_model
from dbx_distributed_pytorch_examples_amd.ops import kernels as K
from dbx_distributed_pytorch_examples_amd.ops import reference as R

pytestmark = pytest.mark.gpu
N, HW, CLASSES, STEPS = 8, 32, 10, 4
ALL_ON = dict(auto_augment="ta_wide", mixup_alpha=0.2, cutmix_alpha=1.0, erase_prob=0.5, erase_mode="pixel")


def dev():
    return torch.device("cuda:0")


def trainer(model=None, **kw):
    if model is None:
        torch.manual_seed(0)
        model = build_model("resnet18", num_classes=CLASSES)
    kw.setdefault("optim", OptimConfig(lr=0.05))
    return NativeTrainer(model, N, (HW, HW), dev(), **kw)


def batches(n, seed=1, integer_boxes=False):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        img = torch.randint(0, 256, (N, HW, HW, 3), dtype=torch.uint8, generator=g)
        lab = torch.randint(0, CLASSES, (N,), generator=g)
        if integer_boxes:  # (unscaled, integer origin: the uint8 image is exact)
            boxes = torch.tensor([[0.0, 0.0, 32.0, 32.0], [2.0, -3.0, 32.0, 32.0]] * (N // 2))
        else:
            boxes = torch.tensor([[1.5, 0.5, 28.0, 30.0], [0.0, 0.0, 32.0, 32.0]] * (N // 2))
        flips = torch.randint(0, 2, (N,), dtype=torch.uint8, generator=g)
        out.append(tuple(t.to(dev()) for t in (img, lab, boxes, flips)))
    return out


def norm(p):
    return p.mean_t.tolist(), p.std_t.tolist()


def test_graph_replay_equals_eager():
    """Graphs against eager, same seed and inputs, with MixUp + CutMix + "pixel" erasing on top: the input and
    the masters are bit-identical after every step."""
    torch.manual_seed(0)
    m1 = build_model("resnet18", num_classes=CLASSES)
    m2 = copy.deepcopy(m1)
    a = trainer(m1, seed=4, label_smoothing=0.1, use_graphs=True, **ALL_ON)
    b = trainer(m2, seed=4, label_smoothing=0.1, use_graphs=False, **ALL_ON)
    for i, bt in enumerate(batches(STEPS, seed=2)):
        a.step(*bt)
        b.step(*bt)
        assert a.last_mix.kind == b.last_mix.kind and a.last_mix["ta"].tolist() == b.last_mix["ta"].tolist()
        assert torch.equal(a.prog.ta_T, b.prog.ta_T) and torch.equal(a.prog.ta_hist, b.prog.ta_hist), i
        assert torch.equal(a.prog.x4, b.prog.x4), i
        assert torch.equal(a.prog.master, b.prog.master), i
    assert a.graphs and all(g is not None for g in a.graphs) and not b.graphs
    s = a.mix_summary()
    assert s["auto_augment"] == "ta_wide" and s["kernel"] == "trivial_augment_u8"


def test_last_mix_is_what_the_kernels_saw():
    """After every step (eager, capture, replay) ``prog.x4`` is bit-equal to a direct ``K.trivial_augment_u8`` call
    with the table ``tr.last_mix["ta"]`` recorded, and the program's T, histograms, LUTs and gray means are
    ``ops/reference.py``'s for it, exactly (integer crop boxes: the uint8 image is exact). With mean 0 and
    std 1 / 255 the input is the augmented uint8 value, so a step without a blend equals the CPU reference's
    input bit for bit; a MixUp step rounds the same real number (both fp32 chains are within 2^-20 of it) to
    bf16 once, so the two differ by at most one bf16 spacing, 2^-7 |ref|."""
    unit = ((0.0, 0.0, 0.0), (1 / 255, 1 / 255, 1 / 255))
    tr = trainer(seed=3, mean=unit[0], std=unit[1], auto_augment="ta_wide",
                 mixup_alpha=0.2, cutmix_alpha=1.0, erase_prob=0.5, erase_mode="const")
    p = tr.prog
    kinds = set()
    for i, b in enumerate(batches(STEPS + 2, integer_boxes=True)):
        tr.step(*b)
        d = tr.last_mix
        kinds.update(d["ta"][:, 0].tolist())
        i32 = lambda a: torch.as_tensor(a, dtype=torch.int32).to(dev())  # noqa: E731
        assert p.ta_ops.tolist() == d["ta"].tolist()
        kw = dict(perm=i32(d.perm), mixbox=i32(list(d.box)), erase=i32(d.erase), erase_mode="const")
        want = torch.full_like(p.x4, float("nan"))
        work = torch.zeros(K.ta_work_words(N, HW, HW), dtype=torch.int32, device=dev())
        K.trivial_augment_u8(p.img_u8, want, p.boxes, *unit, p.flip, i32(d["ta"]), work,
                             blend=torch.tensor([d.blend], device=dev()), **kw)
        assert torch.equal(p.x4, want), (i, d.kind)
        assert torch.equal(p.ta_work, work)
        # the CPU reference, from the program's input buffers and the recorded draw
        c = lambda t: t.cpu()  # noqa: E731
        ref = torch.full(tuple(p.x4.shape), float("nan"), dtype=torch.bfloat16)
        rwork = torch.zeros(K.ta_work_words(N, HW, HW), dtype=torch.int32)
        R.trivial_augment_u8(c(p.img_u8), ref, c(p.boxes), *unit, c(p.flip), torch.from_numpy(d["ta"]), rwork,
                             blend=torch.tensor([d.blend]), **{k: (c(v) if torch.is_tensor(v) else v) for k, v in kw.items()})
        assert torch.equal(c(p.ta_work), rwork), "T, histograms, LUTs and gray means"
        if d.blend == 1.0:
            assert torch.equal(c(p.x4), ref), (i, d.kind)
        else:
            err = (c(p.x4).double() - ref.double()).abs()
            assert bool((err <= 2.0 ** -7 * ref.double().abs()).all()), (i, float(err.max()))
        assert torch.equal(p.labels2, p.labels[i32(d.perm).long()])
    assert len(kinds) >= 4 and tr.graphs


def test_evaluation_never_augments():
    """``eval_step`` and ``evaluate_batch`` write the plain kernel's output, and a validation pass between two
    steps leaves training bit-identical."""
    torch.manual_seed(0)
    m1 = build_model("resnet18", num_classes=CLASSES)
    m2 = copy.deepcopy(m1)
    kw = dict(ALL_ON, seed=6)
    a, b = trainer(m1, **kw), trainer(m2, **kw)
    data = batches(STEPS, seed=5)
    for bt in data[:2]:
        a.step(*bt)
        b.step(*bt)
    p = a.prog
    a.eval_begin()
    for img, lab, boxes, _ in batches(4, seed=7):  # two eager calls, the capture, a replay
        a.eval_step(img, lab, boxes)
        plain = torch.full_like(p.x4, float("nan"))
        K.augment_u8(p.img_u8, plain, p.boxes, *norm(p), p.flip)
        assert torch.equal(p.x4, plain)
    a.eval_end()
    img, lab, boxes, _ = data[0]
    a.evaluate_batch(img, lab, boxes)
    plain = torch.full_like(p.x4, float("nan"))
    K.augment_u8(p.img_u8, plain, p.boxes, *norm(p), p.flip)
    assert torch.equal(p.x4, plain)
    for bt in data[2:]:
        a.step(*bt)
        b.step(*bt)
        assert torch.equal(a.prog.x4, b.prog.x4)
    assert torch.equal(a.prog.master, b.prog.master)


@pytest.mark.parametrize("other", [dict(), dict(mixup_alpha=0.2, erase_prob=0.5)], ids=["plain", "mixing"])
def test_option_off_changes_nothing(other):
    torch.manual_seed(0)
    m1 = build_model("resnet18", num_classes=CLASSES)
    m2 = copy.deepcopy(m1)
    a = trainer(m1, seed=1, auto_augment=None, **other)
    b = trainer(m2, seed=1, **other)
    assert a.prog.ta_ops is None and a.prog.ta_work is None
    assert a.prog.n_wdesc_step == b.prog.n_wdesc_step
    assert (a.prog.mix_arena is None) == (not other) and a.mix_summary()["kernel"] == b.mix_summary()["kernel"] == (
        "augment_mix_u8" if other else "augment_u8")
    for bt in batches(3):
        a.step(*bt)
        b.step(*bt)
        assert torch.equal(a.prog.x4, b.prog.x4)
    assert torch.equal(a.prog.master, b.prog.master)


def test_loss_falls_with_the_option_on():
    torch.manual_seed(0)
    tr = NativeTrainer(build_model("resnet18", num_classes=CLASSES), 64, (HW, HW), dev(),
                       optim=OptimConfig(name="adam", lr=1e-3, weight_decay=0.0), auto_augment="ta_wide")
    img = torch.randint(0, 256, (64, HW, HW, 3), dtype=torch.uint8, device=dev())
    lab = torch.randint(0, CLASSES, (64,), device=dev())
    losses = []
    for i in range(30):
        tr.step(img, lab)
        if i % 10 == 9:
            losses.append(tr.read_metrics()[0] / (10 * 64))
    assert all(l == l for l in losses) and losses[-1] < losses[0], losses
