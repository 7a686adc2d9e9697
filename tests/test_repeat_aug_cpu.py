"""Repeated augmentation: ``parallel.sampler.RepeatAugSampler`` (ShardSampler's permutation, every index repeated
in a row, padded, strided by rank, cut to ShardSampler's length), ``data.aug_repeats`` and its way into both of
train()'s loader paths, and the refusals."""
import math
from collections import Counter

import pytest
import torch

from dbx_distributed_pytorch_examples_amd import config as C
from dbx_distributed_pytorch_examples_amd.parallel.sampler import RepeatAugSampler, ShardSampler

pytestmark = pytest.mark.timeout(600)


@pytest.mark.parametrize("n,world,shuffle,drop_last", [(10, 1, True, False), (10, 3, True, False), (10, 3, True, True),
                                                       (12, 4, False, False), (7, 2, True, True), (1, 4, True, False)])
def test_one_repeat_is_the_shard_sampler(n, world, shuffle, drop_last):
    for epoch in (0, 3):
        for rank in range(world):
            kw = dict(num_replicas=world, rank=rank, shuffle=shuffle, seed=11, drop_last=drop_last)
            a, b = ShardSampler(n, **kw), RepeatAugSampler(n, num_repeats=1, **kw)
            a.set_epoch(epoch)
            b.set_epoch(epoch)
            assert torch.equal(a.indices(), b.indices()) and list(a) == list(b) and len(a) == len(b)


@pytest.mark.parametrize("n,world,r,drop_last", [(10, 1, 3, False), (10, 3, 3, False), (10, 3, 3, True), (100, 8, 3, False),
                                                 (7, 2, 2, True), (9, 4, 5, False), (1, 8, 2, False), (50, 3, 4, True)])
def test_lengths_and_the_epoch_multiset(n, world, r, drop_last):
    base = ShardSampler(n, num_replicas=world, rank=0, seed=4, drop_last=drop_last)
    for epoch in (0, 1):
        base.set_epoch(epoch)
        perm = base.permutation().tolist()
        got = []
        for rank in range(world):
            s = RepeatAugSampler(n, num_repeats=r, num_replicas=world, rank=rank, seed=4, drop_last=drop_last)
            s.set_epoch(epoch)
            idx = s.indices().tolist()
            # the epoch keeps ShardSampler's length on every rank
            assert len(s) == len(idx) == len(list(s)) == base.num_samples == ShardSampler(
                n, num_replicas=world, rank=rank, seed=4, drop_last=drop_last).num_samples
            got += idx
        total = base.num_samples * world
        assert len(got) == total
        # r copies of the first ceil(total / r) permuted ids (the last of them short when r does not divide
        # the total; wrapped around when the dataset is smaller than that)
        rep = [i for i in perm for _ in range(r)]
        want = (rep * math.ceil(total / len(rep)))[:total]
        assert Counter(got) == Counter(want)
        if total <= len(rep):
            ids = perm[:math.ceil(total / r)]
            c = Counter(got)
            assert set(c) == set(ids) and all(c[i] == r for i in ids[:-1]) and c[ids[-1]] == total - r * (len(ids) - 1)


def test_world_three_gives_every_rank_the_same_images():
    per = []
    for rank in range(3):
        s = RepeatAugSampler(30, num_repeats=3, num_replicas=3, rank=rank, seed=2)
        s.set_epoch(5)
        per.append(s.indices().tolist())
    assert per[0] == per[1] == per[2] and len(per[0]) == 10 and len(set(per[0])) == 10
    base = ShardSampler(30, num_replicas=1, rank=0, seed=2)
    base.set_epoch(5)
    assert per[0] == base.permutation().tolist()[:10]  # one third of the images, one copy on each rank


def test_world_one_has_adjacent_copies():
    s = RepeatAugSampler(12, num_repeats=3, num_replicas=1, rank=0, seed=7)
    idx = s.indices().tolist()
    assert len(idx) == 12
    assert all(idx[3 * j] == idx[3 * j + 1] == idx[3 * j + 2] for j in range(4))
    assert len({idx[3 * j] for j in range(4)}) == 4
    s.set_epoch(1)
    assert s.indices().tolist() != idx  # another epoch, another permutation
    e = RepeatAugSampler(6, num_repeats=2, num_replicas=1, rank=0, shuffle=False)
    assert e.indices().tolist() == [0, 0, 1, 1, 2, 2]


class _Streaming:
    """What train() takes for an MDS StreamingDataset: it has ``epoch_indices``."""

    def epoch_indices(self, *a, **kw):
        raise AssertionError("never asked")


@pytest.mark.parametrize("bad", [0, -1, 1.5, "3", True, None])
def test_bad_repeat_counts_are_refused(bad, monkeypatch):
    from dbx_distributed_pytorch_examples_amd.data.datasets import SyntheticImages
    from dbx_distributed_pytorch_examples_amd.train import engine as E
    with pytest.raises(ValueError, match="num_repeats"):
        RepeatAugSampler(10, num_repeats=bad, num_replicas=1, rank=0)
    d = C.DataConfig()
    d.aug_repeats = bad
    with pytest.raises(ValueError, match="aug_repeats"):
        C.validate_data(d)
    with pytest.raises(ValueError, match="aug_repeats"):
        E.make_loader(SyntheticImages(8, 32, 3, 10), 4, True, 0, aug_repeats=bad)
    monkeypatch.setenv("DBX_FORCE_CPU", "1")
    cfg = C.TrainConfig(model="resnet18", num_classes=10, batch_size=4, engine="autograd")
    cfg.data.aug_repeats = bad
    with pytest.raises(ValueError, match="aug_repeats"):
        E.train(cfg, train_dataset=SyntheticImages(8, 32, 3, 10), log_mlflow=False)


def test_a_streaming_dataset_refuses_repeats(monkeypatch):
    from dbx_distributed_pytorch_examples_amd.train import engine as E
    assert E.train_sampler(_Streaming(), 1) is None
    with pytest.raises(ValueError, match="StreamingDataset"):
        E.train_sampler(_Streaming(), 3)
    with pytest.raises(ValueError, match="StreamingDataset"):
        E.make_loader(_Streaming(), 4, True, 0, aug_repeats=2)
    monkeypatch.setenv("DBX_FORCE_CPU", "1")
    cfg = C.TrainConfig(model="resnet18", num_classes=10, batch_size=4, engine="native")
    cfg.data.aug_repeats = 3
    with pytest.raises(ValueError, match="StreamingDataset"):
        E.train(cfg, train_dataset=_Streaming(), log_mlflow=False)


def test_config_field_and_the_a2_file():
    import os
    assert C.DataConfig().aug_repeats == 1 and C.TrainConfig().drop_path_rate == 0.0
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "configs")
    a2 = C.load_config(os.path.join(root, "resnet50_imagenet_8192_a2.yaml"))
    bce = C.load_config(os.path.join(root, "resnet50_imagenet_8192_lamb_bce.yaml"))
    C.validate_train(a2)
    assert (a2.drop_path_rate, a2.data.aug_repeats, a2.data.auto_augment) == (0.05, 3, "ra")
    assert (a2.data.mixup_alpha, a2.data.cutmix_alpha, a2.data.loss, a2.optim.name) == (0.1, 1.0, "bce", "lamb")
    a2.drop_path_rate, a2.data.aug_repeats, a2.data.auto_augment = 0.0, 1, None
    assert C.to_dict(a2) == C.to_dict(bce)  # the LAMB + BCE config plus the three settings, nothing else
    head = open(os.path.join(root, "resnet50_imagenet_8192_a2.yaml")).read().split("model:")[0]
    for words in ("UNTUNED", "per batch", "drop_path_rate", "aug_repeats"):
        assert words in head, words
    over = C.load_config(None, ["data.aug_repeats=2", "drop_path_rate=0.1"])
    assert over.data.aug_repeats == 2 and over.drop_path_rate == 0.1


@pytest.mark.parametrize("engine", ["native", "autograd"])
def test_the_config_reaches_both_loaders(engine, monkeypatch, tmp_path, capsys):
    """train() on the CPU through either loader path: the runner's sampler is the repeat sampler, an epoch keeps its
    length, every image of a batch stream comes r times, and validation is not repeated."""
    from dbx_distributed_pytorch_examples_amd.data.datasets import SyntheticImages
    from dbx_distributed_pytorch_examples_amd.train import engine as E
    monkeypatch.setenv("DBX_FORCE_CPU", "1")
    monkeypatch.setenv("DBX_MLRUNS", str(tmp_path / "mlruns"))
    cfg = C.TrainConfig(model="resnet18", num_classes=10, batch_size=4, epochs=1, log_every=0, engine=engine,
                        graphs=False, seed=3)
    cfg.data.image_size = 32
    cfg.data.num_workers = 0 if engine == "autograd" else 1
    cfg.data.aug_repeats = 2
    cfg.optim.lr = 0.01
    seen = {}
    name = "_Native" if engine == "native" else "_Autograd"
    real = getattr(E, name)

    def spy(*a, **kw):
        r = real(*a, **kw)
        seen["runner"] = r
        return r
    monkeypatch.setattr(E, name, spy)
    evals = []
    real_shard = E.ShardSampler

    def shard_spy(*a, **kw):
        s = real_shard(*a, **kw)
        evals.append(s)
        return s
    monkeypatch.setattr(E, "ShardSampler", shard_spy)
    ds = SyntheticImages(16, 32, 3, 10)  # (uint8 HWC: the native loader's source, and what the collate converts)
    res = E.train(cfg, train_dataset=ds, eval_dataset=SyntheticImages(6, 32, 3, 10, seed=9), log_mlflow=False)
    s = seen["runner"].sampler
    assert type(s) is RepeatAugSampler and s.num_repeats == 2
    assert res.steps == 4 and len(s) == 16  # the epoch's length is the unrepeated one
    idx = s.indices().tolist()
    assert all(idx[2 * j] == idx[2 * j + 1] for j in range(8)) and len(set(idx)) == 8
    assert all(type(e) is ShardSampler for e in evals)  # validation (and only it) built plain samplers
    assert res.history[-1]["val_samples"] == 6
    out = capsys.readouterr().out
    assert out.count("[train] repeated augmentation: aug_repeats=2 sampler=RepeatAugSampler") == 1
