"""The evaluation pass on the GPU: the captured eval forward against the eager ``evaluate_batch`` of a
twin trainer (bit for bit, batch by batch), its device-side metrics against float64 (counts exact, the
loss sum within the derived bound of tests/test_ce_eval.py), one graph for every pass with and without
the weight average, no host sync in a replayed step, training untouched by a pass, and train()."""
import math

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

dev = torch.device("cuda")
SHAPES = {"resnet18": (32, 10), "resnet50": (64, 16)}  # model: (image size, classes)
N = 8


def _batches(n, size, classes, seed=1, last=None):
    g = torch.Generator().manual_seed(seed)
    sizes = [N] * n
    if last is not None:
        sizes[-1] = last
    return [(torch.randint(0, 256, (b, size, size, 3), dtype=torch.uint8, generator=g).to(dev),
             torch.randint(0, classes, (b,), generator=g).to(dev)) for b in sizes]


def _trainer(name, model=None, **kw):
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig
    from dbx_distributed_pytorch_examples_amd.models import build_model
    size, classes = SHAPES[name]
    if model is None:
        torch.manual_seed(0)
        model = build_model(name, num_classes=classes)
    return NativeTrainer(model, N, (size, size), dev, optim=OptimConfig(lr=0.05), **kw)


def _twin(name, a, **kw):
    """An eager trainer holding a's parameters, running statistics and (if any) average."""
    from dbx_distributed_pytorch_examples_amd.models import build_model
    m = build_model(name, num_classes=SHAPES[name][1])
    m.load_state_dict(a.prog.model.state_dict())
    b = _trainer(name, m, use_graphs=False, **kw)
    _follow(a, b)
    return b


def _follow(a, b):
    b.prog.model.load_state_dict(a.prog.model.state_dict())
    assert torch.equal(b.prog.master, a.prog.master)
    if a.ema is not None:
        b.ema.copy_(a.ema)
        b.ema_bn.copy_(a.ema_bn)


def metrics64(logits, labels, k):
    """float64 (loss sum, top-1, top-k, bound of the loss sum) of a logits matrix as read (bf16 is exact):
    per row 2^-20 (|lse| + |x_l|), plus (n 2^-24 + 2^-21) sum |loss| for the sum of n fp32 terms."""
    x, labels = logits.double().cpu(), labels.cpu()
    xl = x.gather(1, labels[:, None])
    idx = torch.arange(x.shape[1])[None, :]
    rank = ((x > xl) | ((x == xl) & (idx < labels[:, None]))).sum(1)
    mx = x.max(1, keepdim=True).values
    lse = (mx + torch.log(torch.exp(x - mx).sum(1, keepdim=True))).squeeze(1)
    loss = lse - xl.squeeze(1)
    n = x.shape[0]
    bound = 2.0 ** -20 * (lse.abs() + xl.squeeze(1).abs()).sum() + (n * 2.0 ** -24 + 2.0 ** -21) * loss.abs().sum()
    return float(loss.sum()), float((rank < 1).sum()), float((rank < k).sum()), float(bound)


def check_pass(a, b, data, use_ema, k, classes, no_sync_from=None):
    """One pass of ``a`` over ``data`` against ``b.evaluate_batch``, after every call and in total."""
    tot = [0.0, 0.0, 0.0, 0.0]
    a.eval_begin(use_ema=use_ema, topk=k)
    for i, (x, y) in enumerate(data):
        if no_sync_from is not None and i >= no_sync_from:
            assert a.eval_graph is not None
            torch.cuda.set_sync_debug_mode("error")
            try:
                a.eval_step(x, y)
            finally:
                torch.cuda.set_sync_debug_mode("default")
        else:
            a.eval_step(x, y)
        want = b.evaluate_batch(x, y, use_ema=use_ema)
        assert torch.equal(a.prog.logits[:x.shape[0]], want), f"batch {i}"
        tot = [s + t for s, t in zip(tot, metrics64(want, y, min(k, classes)))]
    r = a.eval_end()
    n = sum(y.shape[0] for _, y in data)
    assert (r.top1, r.topk, r.count, r.k) == (tot[1], tot[2], n, min(k, classes))
    err = abs(r.loss_sum - tot[0])
    print(f"eval pass loss sum: err / bound = {err / tot[3]:.4f}")
    assert err <= tot[3], (r.loss_sum, tot[0], tot[3])
    return r


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_graph_against_eager(name):
    size, classes = SHAPES[name]
    a = _trainer(name)
    for x, y in _batches(3, size, classes):
        a.step(x, y)
    b = _twin(name, a)
    # two eager calls, the capture, two replays (no host sync in them), the last batch short
    check_pass(a, b, _batches(5, size, classes, seed=5, last=3), None, 5, classes, no_sync_from=3)
    g = a.eval_graph
    assert g is not None
    # a second pass after one more training step replays the same graph on the new weights
    a.step(*_batches(1, size, classes, seed=6)[0])
    _follow(a, b)
    check_pass(a, b, _batches(2, size, classes, seed=7, last=5), None, 5, classes, no_sync_from=0)
    assert a.eval_graph is g
    assert torch.equal(a.eval_nvalid.cpu(), torch.tensor([5], dtype=torch.int32))


def test_one_graph_with_and_without_the_average():
    name = "resnet18"
    size, classes = SHAPES[name]
    a = _trainer(name, ema_decay=0.9)
    for x, y in _batches(3, size, classes):
        a.step(x, y)
    assert not torch.equal(a.ema, a.prog.master)
    b = _twin(name, a, ema_decay=0.9)
    data = _batches(3, size, classes, seed=5, last=1)
    on = check_pass(a, b, data, True, 5, classes)
    g = a.eval_graph
    assert g is not None
    off = check_pass(a, b, data, False, 5, classes, no_sync_from=0)
    dflt = check_pass(a, b, data, None, 5, classes, no_sync_from=0)  # None: the average when there is one
    assert a.eval_graph is g and (dflt.top1, dflt.topk, dflt.count) == (on.top1, on.topk, on.count)
    # (the same fp32 losses, added by fp64 atomics in another order)
    assert abs(dflt.loss_sum - on.loss_sum) <= 2.0 ** -45 * abs(on.loss_sum) and on.loss_sum != off.loss_sum
    plain = _trainer(name, use_graphs=False)
    with pytest.raises(ValueError, match="ema_decay"):
        plain.eval_begin(use_ema=True)
    for call in (lambda: plain.eval_step(*data[0]), plain.eval_end):
        with pytest.raises(RuntimeError):
            call()
    plain.eval_begin()
    for call in (plain.eval_begin, lambda: plain.step(*data[0])):
        with pytest.raises(RuntimeError):
            call()
    plain.eval_end()


@pytest.mark.parametrize("ema_decay", [0.0, 0.9])
def test_training_is_untouched(ema_decay):
    name = "resnet18"
    size, classes = SHAPES[name]
    a, b = _trainer(name, ema_decay=ema_decay), _trainer(name, ema_decay=ema_decay)
    assert torch.equal(a.prog.master, b.prog.master)
    ev = _batches(3, size, classes, seed=9, last=2)
    for i, (x, y) in enumerate(_batches(5, size, classes, seed=3)):
        if i == 3:  # between steps 3 and 4: two eager calls and the capture + replay
            a.eval_begin()
            for xe, ye in ev:
                a.eval_step(xe, ye)
            assert a.eval_end().count == 2 * N + 2
        a.step(x, y)
        b.step(x, y)
    torch.cuda.synchronize()
    assert torch.equal(a.prog.master, b.prog.master) and torch.equal(a.mom, b.mom)
    assert torch.equal(a.prog.metrics, b.prog.metrics)
    if ema_decay > 0:
        assert torch.equal(a.ema, b.ema) and torch.equal(a.ema_bn, b.ema_bn)


def test_train_end_to_end(tmp_path, monkeypatch):
    monkeypatch.setenv("DBX_MLRUNS", str(tmp_path / "mlruns"))
    import numpy as np

    from dbx_distributed_pytorch_examples_amd.config import TrainConfig
    from dbx_distributed_pytorch_examples_amd.data.datasets import SyntheticImages
    from dbx_distributed_pytorch_examples_amd.train import engine as E
    tr_ds, ev_ds = SyntheticImages(128, 32, 3, 10, seed=1), SyntheticImages(64, 32, 3, 10, seed=2)
    img = torch.from_numpy(np.stack([ev_ds[i][0] for i in range(64)])).to(dev)
    lab = torch.tensor([int(ev_ds[i][1]) for i in range(64)], device=dev)

    def run(mags=None, **kw):
        cfg = TrainConfig(model="resnet18", num_classes=10, batch_size=32, epochs=2, log_every=0, **kw)
        cfg.data.image_size = 32
        cfg.optim.lr = 0.02

        def largest_logit(epoch, rec, runner):  # of the validation set, at this epoch's weights
            mags.append(max(float(runner.tr.evaluate_batch(img[lo:lo + 32], lab[lo:lo + 32]).float().abs().max())
                            for lo in (0, 32)))

        return E.train(cfg, train_dataset=tr_ds, eval_dataset=ev_ds, log_mlflow=False,
                       callbacks=[largest_logit] if mags is not None else None)

    mags = []
    res = run(mags)
    assert res.engine == "native" and res.steps == 8 and len(res.history) == 2
    for h in res.history:
        assert h["val_samples"] == 64 and math.isfinite(h["val_loss"])
        assert h["val_accuracy"] <= h["val_top5_accuracy"] <= 1.0
    # the host path (torch's CE on the fp32 logits): the same counts; each mean loss is within the plain
    # fp32 bound of the exact one -- per row 2^-20 (|lse| + |x_l|) <= 2^-20 (ln C + 2 max |x|), plus the
    # sum of 64 fp32 terms -- so the two differ by at most twice that
    host = run(eval_graph=False)
    for h, g, mag in zip(host.history, res.history, mags):
        assert h["val_accuracy"] == g["val_accuracy"] and h["val_top5_accuracy"] == g["val_top5_accuracy"]
        assert h["train_loss"] == g["train_loss"]
        bound = 2 * (2.0 ** -20 * (math.log(10) + 2 * mag)
                     + (64 * 2.0 ** -24 + 2.0 ** -21) * max(h["val_loss"], g["val_loss"]))
        err = abs(h["val_loss"] - g["val_loss"])
        print(f"val_loss, host path against the pass: err / bound = {err / bound:.4f}")
        assert err <= bound, (h["val_loss"], g["val_loss"], bound)
    off = run(eval_topk=0)
    assert all(not any(k.startswith("val_top") for k in h) and "val_accuracy" in h for h in off.history)
