"""Ragged input batches inside the native training step, on the GPU: ResNet-18, 10 classes, batch 16, 32x32.
A ragged trainer fed equal-size batches is the dense trainer bit for bit; a replayed graph follows new bytes
and a new table through static addresses; what the step feeds the network is the standalone ragged kernel call;
evaluation takes short batches and never augments; what a ragged trainer cannot take is refused."""
import copy

import numpy as np
import pytest
import torch

from dbx_distributed_pytorch_examples_amd.data.loader import pack_images, ragged_capacity
from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig
from dbx_distributed_pytorch_examples_amd.engine.program import ResNetProgram
from dbx_distributed_pytorch_examples_amd.models import build_model
from dbx_distributed_pytorch_examples_amd.ops import kernels as K

pytestmark = pytest.mark.gpu
N, HW, CLASSES = 16, 32, 10
MAX_HW = (48, 64)
SIZES = [(32, 32), (40, 52), (33, 47), (48, 36), (37, 64), (9, 11), (48, 64), (1, 1)]


def dev():
    return torch.device("cuda:0")


def models():
    torch.manual_seed(0)
    m = build_model("resnet18", num_classes=CLASSES)
    return m, copy.deepcopy(m)


def trainer(model, **kw):
    kw.setdefault("optim", OptimConfig(lr=0.05))
    return NativeTrainer(model, N, (HW, HW), dev(), **kw)


def ragged_batches(n, seed=1, uniform=None, count=N):
    """[(packed, labels, boxes, flips, table)] on the device, sizes cycling through SIZES from a different start
    each step (``uniform``: every image of that size), with the images as a list (numpy)."""
    rs = np.random.default_rng(seed)
    out = []
    for s in range(n):
        shapes = [uniform or SIZES[(s + k) % len(SIZES)] for k in range(count)]
        imgs = [rs.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
        arena, table = pack_images(imgs, 3)
        boxes = np.array([(0.3, 0.6, 0.8 * h + 0.1, 0.9 * w) for h, w in shapes], np.float32)
        t = (torch.from_numpy(arena.copy()), torch.from_numpy(rs.integers(0, CLASSES, count)),
             torch.from_numpy(boxes), torch.from_numpy(rs.integers(0, 2, count).astype(np.uint8)), torch.from_numpy(table))
        out.append((tuple(x.to(dev()) for x in t), imgs))
    return out


def norm(p):
    return p.mean_t.tolist(), p.std_t.tolist()


def test_program_buffers():
    m, _ = models()
    p = ResNetProgram(m, N, (HW, HW), dev(), src_ragged=MAX_HW)
    assert p.img_u8.dim() == 1 and p.img_u8.numel() == ragged_capacity(N, MAX_HW, 3) == N * 48 * 192
    assert p.src_tab.dtype == torch.int32 and p.src_tab.tolist() == [[0, 1, 1, 16]] * N
    assert ResNetProgram(copy.deepcopy(m), N, (HW, HW), dev()).src_tab is None
    with pytest.raises(ValueError, match="exclude"):
        ResNetProgram(m, N, (HW, HW), dev(), src_hw=(40, 40), src_ragged=MAX_HW)


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graphs"])
def test_equal_sizes_are_the_dense_trainer(graphs):
    m1, m2 = models()
    a = trainer(m1, src_ragged=MAX_HW, use_graphs=graphs, label_smoothing=0.1)
    b = trainer(m2, src_hw=(40, 52), use_graphs=graphs, label_smoothing=0.1)
    for i, ((packed, lab, boxes, flips, table), imgs) in enumerate(ragged_batches(3 + 2 * graphs, uniform=(40, 52))):
        dense = torch.from_numpy(np.stack(imgs)).to(dev())
        a.step(packed, lab, boxes, flips, src_table=table)
        b.step(dense, lab, boxes, flips)
        assert torch.equal(a.prog.x4, b.prog.x4), i
        assert torch.equal(a.prog.master, b.prog.master), i
        assert a.read_metrics() == b.read_metrics(), i
    assert bool(a.graphs) == graphs


@pytest.mark.parametrize("opts", [dict(), dict(auto_augment="ra", mixup_alpha=0.2, erase_prob=0.5, erase_mode="pixel")],
                         ids=["plain", "ra-mixup-erase"])
def test_graph_replay_follows_new_bytes_and_a_new_table(opts):
    """Six steps (two eager warm-ups, the capture, three replays), a different packing each: graphs equal eager bit
    for bit, and ``prog.x4`` is the standalone ragged call on the step's arena, table and sampled options."""
    m1, m2 = models()
    a = trainer(m1, src_ragged=MAX_HW, seed=4, use_graphs=True, **opts)
    b = trainer(m2, src_ragged=MAX_HW, seed=4, use_graphs=False, **opts)
    p = a.prog
    ptrs = (p.img_u8.data_ptr(), p.src_tab.data_ptr())
    tables = set()
    for i, ((packed, lab, boxes, flips, table), _) in enumerate(ragged_batches(6, seed=2)):
        a.step(packed, lab, boxes, flips, src_table=table)
        b.step(packed, lab, boxes, flips, src_table=table)
        tables.add(tuple(table.flatten().tolist()))
        assert torch.equal(p.x4, b.prog.x4), i
        assert torch.equal(p.master, b.prog.master), i
        assert torch.equal(p.src_tab, table) and torch.equal(p.img_u8[:packed.numel()], packed)
        want = torch.full_like(p.x4, float("nan"))
        if opts:
            kw = dict(perm=p.mix_perm, mixbox=p.mix_box, blend=p.mix_blend, erase=p.erase_box, erase_mode="pixel",
                      erase_rng=(p.erase_seed, p.erase_off.clone()))
            work = torch.zeros(K.ta_work_words(N, HW, HW, 2), dtype=torch.int32, device=dev())
            K.chain_augment_u8(p.img_u8, want, p.boxes, *norm(p), p.flip, p.ta_ops.reshape(2, N, 8), work, src=p.src_tab,
                               **kw)
        else:
            K.augment_u8(p.img_u8, want, p.boxes, *norm(p), p.flip, src=p.src_tab)
        assert torch.equal(p.x4, want), i
    assert a.graphs and not b.graphs and len(tables) == 6
    assert ptrs == (p.img_u8.data_ptr(), p.src_tab.data_ptr()), "static addresses"


def test_eval_takes_short_batches_and_never_augments():
    m1, m2 = models()
    a = trainer(m1, src_ragged=MAX_HW, seed=6, auto_augment="ra", mixup_alpha=0.2, erase_prob=0.5)
    b = trainer(m2, src_ragged=MAX_HW, seed=6)
    data = ragged_batches(3, seed=5)
    for (packed, lab, boxes, flips, table), _ in data:
        a.step(packed, lab, boxes, flips, src_table=table)
    m2.load_state_dict(m1.state_dict())
    b.params_changed()
    n = 11
    (packed, lab, boxes, _, table), imgs = ragged_batches(1, seed=8, count=n)[0]
    la = a.evaluate_batch(packed, lab, boxes, src_table=table)
    lb = b.evaluate_batch(packed, lab, boxes, src_table=table)
    assert la.shape[0] == n and torch.equal(la, lb)
    assert torch.equal(a.prog.x4[:n], b.prog.x4[:n]), "(rows at or past n keep what each trainer held)"
    plain = torch.full_like(a.prog.x4, float("nan"))
    K.augment_u8(a.prog.img_u8, plain, a.prog.boxes, *norm(a.prog), a.prog.flip, src=a.prog.src_tab)
    assert torch.equal(a.prog.x4, plain), "no flip, no operation, no mixing"
    # row k < n is the dense evaluation of that image alone
    for k in (0, 5, n - 1):
        one = torch.full((1, HW, HW, 4), float("nan"), dtype=torch.bfloat16, device=dev())
        K.augment_u8(torch.from_numpy(imgs[k][None]).to(dev()), one, boxes[k:k + 1], *norm(a.prog))
        assert torch.equal(a.prog.x4[k], one[0]), k
    # the prepared pass: two eager calls, the capture, a replay; a short batch counts its n samples only
    a.eval_begin()
    b.eval_begin()
    total = 0
    for i, cnt in enumerate((N, n, N, 5)):
        (packed, lab, boxes, _, table), _ = ragged_batches(1, seed=20 + i, count=cnt)[0]
        a.eval_step(packed, lab, boxes, src_table=table)
        b.eval_step(packed, lab, boxes, src_table=table)
        assert torch.equal(a.prog.x4[:cnt], b.prog.x4[:cnt]), i
        total += cnt
    ra, rb = a.eval_end(), b.eval_end()
    assert ra == rb and ra.count == total


def test_refusals():
    m1, m2 = models()
    a = trainer(m1, src_ragged=MAX_HW)
    d = trainer(m2)
    (packed, lab, boxes, flips, table), imgs = ragged_batches(1, uniform=(32, 32))[0]
    dense = torch.from_numpy(np.stack(imgs)).to(dev())
    with pytest.raises(ValueError, match="packed 1-D"):
        a.step(dense, lab, boxes, flips, src_table=table)
    with pytest.raises(ValueError, match="src_table"):
        a.step(packed, lab, boxes, flips)
    with pytest.raises(ValueError, match="src_table"):
        a.step(None, lab, src_table=table)
    with pytest.raises(TypeError):
        a.step(packed, lab, boxes, flips, src_table=table.long())
    with pytest.raises(ValueError):
        a.step(packed, lab, boxes, flips, src_table=table[:N - 1])
    with pytest.raises(ValueError, match="holds"):
        a.step(torch.zeros(a.prog.img_u8.numel() + 16, dtype=torch.uint8, device=dev()), lab, boxes, flips,
               src_table=table)
    with pytest.raises(ValueError, match="ragged trainer"):
        d.step(dense, lab, boxes, flips, src_table=table)
    with pytest.raises(ValueError, match="ragged trainer"):
        d.evaluate_batch(dense, lab, boxes, src_table=table)
    with pytest.raises(ValueError, match="exclude"):
        trainer(m2, src_hw=(32, 32), src_ragged=MAX_HW)
    a.step(packed, lab, boxes, flips, src_table=table)  # (and this is accepted)
    d.step(dense, lab, boxes, flips)
    assert torch.equal(a.prog.x4, d.prog.x4)
