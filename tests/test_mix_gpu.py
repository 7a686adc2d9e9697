"""MixUp, the MixUp / CutMix switch and random erasing inside the native training step, on the GPU:
ResNet-18, 10 classes, batch 16, 32x32. What the captured step feeds the network is the mixing kernel's
output for what the host sampled; a replayed graph follows every scalar, table and the Philox offset;
evaluation never mixes or erases; with the options off nothing changes."""
import copy

import pytest
import torch

from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig
from dbx_distributed_pytorch_examples_amd.models import build_model
from dbx_distributed_pytorch_examples_amd.ops import kernels as K

pytestmark = pytest.mark.gpu
N, HW, CLASSES = 16, 32, 10
ALL_ON = dict(mixup_alpha=0.2, cutmix_alpha=1.0, erase_prob=0.5, erase_mode="pixel")


def dev():
    return torch.device("cuda:0")


def trainer(model=None, **kw):
    if model is None:
        torch.manual_seed(0)
        model = build_model("resnet18", num_classes=CLASSES)
    kw.setdefault("optim", OptimConfig(lr=0.05))
    return NativeTrainer(model, N, (HW, HW), dev(), **kw)


def batches(n, seed=1):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        img = torch.randint(0, 256, (N, HW, HW, 3), dtype=torch.uint8, generator=g)
        lab = torch.randint(0, CLASSES, (N,), generator=g)
        boxes = torch.tensor([[1.5, 0.5, 28.0, 30.0], [0.0, 0.0, 32.0, 32.0]] * (N // 2))
        flips = torch.randint(0, 2, (N,), dtype=torch.uint8, generator=g)
        out.append(tuple(t.to(dev()) for t in (img, lab, boxes, flips)))
    return out


def norm(p):
    return p.mean_t.tolist(), p.std_t.tolist()


def test_wiring_the_step_feeds_the_kernels_output():
    """Eager warm-ups, the capture and replays: after every step ``prog.x4`` is bit-equal to a direct
    ``K.augment_u8`` call with what ``tr.last_mix`` recorded and the program's input buffers."""
    tr = trainer(seed=3, **ALL_ON)
    p = tr.prog
    kinds, erased = set(), 0
    for i, b in enumerate(batches(8)):
        tr.step(*b)
        d = tr.last_mix
        kinds.add(d.kind)
        erased += int((d.erase[:, 1] > d.erase[:, 0]).sum())
        i32 = lambda a: torch.as_tensor(a, dtype=torch.int32).to(dev())  # noqa: E731
        assert int(p.erase_off) == i + 1, "the offset advances by one per step, on the device"
        want = torch.full_like(p.x4, float("nan"))
        K.augment_u8(p.img_u8, want, p.boxes, *norm(p), p.flip, perm=i32(d.perm), mixbox=i32(list(d.box)),
                     blend=torch.tensor([d.blend], device=dev()), erase=i32(d.erase), erase_mode="pixel",
                     erase_rng=(p.erase_seed, i32([i + 1])))
        assert torch.equal(p.x4, want), (i, d.kind)
        assert torch.equal(p.labels2, p.labels[i32(d.perm).long()])
        assert float(p.mix_lam) == float(torch.tensor(d.lam, dtype=torch.float32))
    assert kinds == {"mixup", "cutmix"} and erased > 0 and tr.graphs


def test_graph_replay_follows_every_scalar():
    """Graphs against eager, same seed and inputs, 6 steps (two eager warm-ups, the capture, replays): the
    masters are bit-identical after every step."""
    torch.manual_seed(0)
    m1 = build_model("resnet18", num_classes=CLASSES)
    m2 = copy.deepcopy(m1)
    a = trainer(m1, seed=4, label_smoothing=0.1, use_graphs=True, **ALL_ON)
    b = trainer(m2, seed=4, label_smoothing=0.1, use_graphs=False, **ALL_ON)
    for i, bt in enumerate(batches(6, seed=2)):
        a.step(*bt)
        b.step(*bt)
        assert a.last_mix.kind == b.last_mix.kind and a.last_mix.lam == b.last_mix.lam
        assert torch.equal(a.prog.x4, b.prog.x4), i
        assert torch.equal(a.prog.master, b.prog.master), i
    assert int(a.prog.erase_off) == int(b.prog.erase_off) == 6
    assert a.graphs and all(g is not None for g in a.graphs) and not b.graphs


def test_graph_replay_with_accumulation_advances_the_offset():
    """grad_accum 2: the micro graph and the boundary graph both advance the Philox offset."""
    torch.manual_seed(0)
    m1 = build_model("resnet18", num_classes=CLASSES)
    m2 = copy.deepcopy(m1)
    a = trainer(m1, seed=4, grad_accum=2, use_graphs=True, **ALL_ON)
    b = trainer(m2, seed=4, grad_accum=2, use_graphs=False, **ALL_ON)
    for i, bt in enumerate(batches(8, seed=3)):
        a.step(*bt)
        b.step(*bt)
        assert int(a.prog.erase_off) == i + 1
        assert torch.equal(a.prog.x4, b.prog.x4), i
    assert torch.equal(a.prog.master, b.prog.master)
    assert a.graphs and a.micro_graphs


def test_loss_falls_with_all_options_on():
    torch.manual_seed(0)
    tr = NativeTrainer(build_model("resnet18", num_classes=CLASSES), 64, (HW, HW), dev(),
                       optim=OptimConfig(name="adam", lr=1e-3, weight_decay=0.0), label_smoothing=0.1,
                       mixup_alpha=0.2, cutmix_alpha=1.0, erase_prob=0.25, erase_mode="pixel")
    img = torch.randint(0, 256, (64, HW, HW, 3), dtype=torch.uint8, device=dev())
    lab = torch.randint(0, CLASSES, (64,), device=dev())
    losses = []
    for i in range(30):
        tr.step(img, lab)
        if i % 10 == 9:
            losses.append(tr.read_metrics()[0] / (10 * 64))
    assert all(l == l for l in losses) and losses[-1] < losses[0], losses


def test_options_off_change_nothing():
    torch.manual_seed(0)
    m1 = build_model("resnet18", num_classes=CLASSES)
    m2 = copy.deepcopy(m1)
    a = trainer(m1, seed=1, mixup_alpha=0.0, erase_prob=0.0)
    b = trainer(m2, seed=1)
    assert a.prog.mix_blend is None and a.prog.erase_box is None and a.prog.mix_perm is None
    assert a.prog.n_wdesc_step == b.prog.n_wdesc_step
    for bt in batches(4):
        a.step(*bt)
        b.step(*bt)
    assert torch.equal(a.prog.master, b.prog.master)


def test_evaluation_never_mixes_or_erases():
    """``eval_step`` (eager calls, then the captured graph) and ``evaluate_batch`` write the plain kernel's
    output, and a validation pass between two steps leaves training bit-identical."""
    torch.manual_seed(0)
    m1 = build_model("resnet18", num_classes=CLASSES)
    m2 = copy.deepcopy(m1)
    kw = dict(mixup_alpha=0.2, cutmix_alpha=1.0, erase_prob=1.0, erase_mode="pixel", seed=6)
    a, b = trainer(m1, **kw), trainer(m2, **kw)
    data = batches(4, seed=5)
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
    assert int(p.erase_off) == 2, "evaluation does not advance the offset"
    for bt in data[2:]:
        a.step(*bt)
        b.step(*bt)
    assert torch.equal(a.prog.master, b.prog.master)
