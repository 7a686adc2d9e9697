"""The evaluation pass (NativeTrainer.eval_begin / eval_step / eval_end) on the CPU reference ops, and
train() reporting top-k validation accuracy on the native and the autograd engine.

The pass's counts are compared exactly and its loss sum within the derived bound of
tests/test_ce_eval.py against float64 metrics of ``evaluate_batch``'s logits: per row
``2^-20 (|lse| + |x_l|)``, plus ``(n 2^-24 + 2^-21) sum |loss|`` for the sum of n fp32 terms.
"""
import copy
import math

import pytest
import torch

pytestmark = pytest.mark.timeout(600)

CPU = torch.device("cpu")
N, SIZE, CLASSES = 4, 32, 10


def _batches(n, batch=N, seed=1, last=None):
    g = torch.Generator().manual_seed(seed)
    sizes = [batch] * n
    if last is not None:
        sizes[-1] = last
    return [(torch.randint(0, 256, (b, SIZE, SIZE, 3), dtype=torch.uint8, generator=g),
             torch.randint(0, CLASSES, (b,), generator=g)) for b in sizes]


def _trainer(model, **kw):
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig
    return NativeTrainer(model, N, (SIZE, SIZE), CPU, optim=OptimConfig(lr=0.05), use_graphs=False, **kw)


def _model():
    from dbx_distributed_pytorch_examples_amd.models import build_model
    torch.manual_seed(0)
    return build_model("resnet18", num_classes=CLASSES)


def metrics64(logits, labels, k):
    """float64 (loss sum, top-1, top-k, bound of the loss sum) of a logits matrix as read (bf16 is exact)."""
    x = logits.double()
    xl = x.gather(1, labels[:, None])
    idx = torch.arange(x.shape[1])[None, :]
    rank = ((x > xl) | ((x == xl) & (idx < labels[:, None]))).sum(1)
    mx = x.max(1, keepdim=True).values
    lse = (mx + torch.log(torch.exp(x - mx).sum(1, keepdim=True))).squeeze(1)
    loss = lse - xl.squeeze(1)
    n = x.shape[0]
    bound = 2.0 ** -20 * (lse.abs() + xl.squeeze(1).abs()).sum() + (n * 2.0 ** -24 + 2.0 ** -21) * loss.abs().sum()
    return float(loss.sum()), float((rank < 1).sum()), float((rank < k).sum()), float(bound)


def check_pass(tr, data, use_ema, k, want_ema=None):
    """Run one pass over ``data``; compare with evaluate_batch's logits, batch by batch and in total."""
    want_ema = use_ema if want_ema is None else want_ema
    ref = [tr.evaluate_batch(x, y, use_ema=want_ema).clone() for x, y in data]
    tot = [0.0, 0.0, 0.0, 0.0]
    for lg, (_, y) in zip(ref, data):
        tot = [a + b for a, b in zip(tot, metrics64(lg, y, min(k, CLASSES)))]
    tr.eval_begin(use_ema=use_ema, topk=k)
    for lg, (x, y) in zip(ref, data):
        tr.eval_step(x, y)
        assert torch.equal(tr.prog.logits[:x.shape[0]], lg)
    r = tr.eval_end()
    n = sum(y.shape[0] for _, y in data)
    assert (r.top1, r.topk, r.count, r.k) == (tot[1], tot[2], n, min(k, CLASSES))
    err = abs(r.loss_sum - tot[0])
    print(f"eval pass loss sum: err / bound = {err / tot[3]:.4f}")
    assert err <= tot[3], (r.loss_sum, tot[0], tot[3])
    assert r.top1 <= r.topk <= r.count
    return r


def test_pass_matches_evaluate_batch():
    tr = _trainer(_model())
    for x, y in _batches(2):
        tr.step(x, y)
    data = _batches(3, seed=5, last=3)
    r5 = check_pass(tr, data, None, 5)
    r1 = check_pass(tr, data, False, 1)
    assert r1.topk == r1.top1 == r5.top1 and r1.loss_sum == r5.loss_sum
    r99 = check_pass(tr, data, None, 99)  # clipped to the class count: every counted row is a hit
    assert r99.k == CLASSES and r99.topk == r99.count == 11
    # the pass owns its sums: the training metrics are untouched
    before = tr.prog.metrics.clone()
    check_pass(tr, data, None, 5)
    assert torch.equal(tr.prog.metrics, before)


def test_pass_with_the_average():
    tr = _trainer(_model(), ema_decay=0.5)
    for x, y in _batches(3):
        tr.step(x, y)
    assert not torch.equal(tr.ema, tr.prog.master)
    data = _batches(3, seed=5, last=1)
    on = check_pass(tr, data, True, 5)
    off = check_pass(tr, data, False, 5)
    dflt = check_pass(tr, data, None, 5, want_ema=True)  # None: the average when there is one
    assert dflt == on and on.loss_sum != off.loss_sum
    plain = _trainer(_model())
    check_pass(plain, data, None, 5, want_ema=False)
    with pytest.raises(ValueError, match="ema_decay"):
        plain.eval_begin(use_ema=True)
    plain.eval_begin()  # (the refused call opened no pass)
    plain.eval_end()


def test_state_errors():
    tr = _trainer(_model())
    (x, y), = _batches(1)
    with pytest.raises(RuntimeError):
        tr.eval_step(x, y)
    with pytest.raises(RuntimeError):
        tr.eval_end()
    tr.eval_begin()
    with pytest.raises(RuntimeError):
        tr.eval_begin()
    with pytest.raises(RuntimeError):
        tr.step(x, y)
    with pytest.raises(ValueError):
        tr.eval_step(torch.cat([x, x]), torch.cat([y, y]))  # more rows than the program's batch
    tr.eval_step(x, y)
    assert tr.eval_end().count == N
    with pytest.raises(RuntimeError):
        tr.eval_end()
    with pytest.raises(ValueError):
        tr.eval_begin(topk=0)
    tr.step(x, y)  # closed: training goes on


@pytest.mark.parametrize("ema_decay", [0.0, 0.9])
def test_training_is_untouched(ema_decay):
    m = _model()
    a, b = _trainer(m, ema_decay=ema_decay), _trainer(copy.deepcopy(m), ema_decay=ema_decay)
    data = _batches(5, seed=3)
    ev = _batches(2, seed=9, last=2)
    for i, (x, y) in enumerate(data):
        if i == 3:
            a.eval_begin()
            for xe, ye in ev:
                a.eval_step(xe, ye)
            assert a.eval_end().count == 6
        a.step(x, y)
        b.step(x, y)
    assert torch.equal(a.prog.master, b.prog.master) and torch.equal(a.mom, b.mom)
    assert torch.equal(a.prog.metrics, b.prog.metrics)
    if ema_decay > 0:
        assert torch.equal(a.ema, b.ema) and torch.equal(a.ema_bn, b.ema_bn)


def test_forward_switches_keep_their_defaults():
    """forward(loss=False, bn_coeffs=False) after bn_eval_coeffs() gives the logits of the plain eval forward."""
    tr = _trainer(_model())
    (x, y), = _batches(1)
    tr.step(x, y)
    want = tr.evaluate_batch(x, y).clone()
    p = tr.prog
    p.bn_arena.fill_(float("nan"))
    p.logits.zero_()
    p.prepare_weights()
    p.bn_eval_coeffs()
    p.training = False
    try:
        p.load_input_u8(None)
        out = p.forward(compute_grad=False, metrics=False, loss=False, bn_coeffs=False)
    finally:
        p.training = True
    assert torch.equal(out, want)


# ---------------------------------------------------------------------------------------------
# train()
# ---------------------------------------------------------------------------------------------
def _cfg(engine="native", **kw):
    from dbx_distributed_pytorch_examples_amd.config import TrainConfig
    cfg = TrainConfig(model="resnet18", num_classes=CLASSES, batch_size=N, epochs=2, log_every=0, engine=engine,
                      graphs=False, **kw)
    cfg.data.image_size = SIZE
    cfg.data.num_workers = 1
    cfg.optim.lr = 0.02
    return cfg


def _train(monkeypatch, tmp_path, mags=None, **kw):
    """train() for two epochs of two steps with six validation samples (a full and a short batch).
    ``mags``: a list that receives, per epoch, the largest |logit| of the validation set."""
    import numpy as np
    monkeypatch.setenv("DBX_MLRUNS", str(tmp_path / "mlruns"))
    monkeypatch.setenv("DBX_FORCE_CPU", "1")
    from dbx_distributed_pytorch_examples_amd.data.datasets import SyntheticImages
    from dbx_distributed_pytorch_examples_amd.train.engine import train
    tr_ds, ev_ds = SyntheticImages(8, SIZE, 3, CLASSES, seed=1), SyntheticImages(6, SIZE, 3, CLASSES, seed=2)

    def largest_logit(epoch, rec, runner):
        img = torch.from_numpy(np.stack([ev_ds[i][0] for i in range(6)]))
        lab = torch.tensor([int(ev_ds[i][1]) for i in range(6)])
        mags.append(max(float(runner.tr.evaluate_batch(img[lo:hi], lab[lo:hi]).float().abs().max())
                        for lo, hi in ((0, N), (N, 6))))

    return train(_cfg(**kw), train_dataset=tr_ds, eval_dataset=ev_ds, log_mlflow=False,
                 callbacks=[largest_logit] if mags is not None else None)


def test_config_keys():
    from dbx_distributed_pytorch_examples_amd.config import TrainConfig, load_config
    assert (TrainConfig().eval_topk, TrainConfig().eval_graph) == (5, True)
    cfg = load_config(None, ["eval_topk=3", "eval_graph=false"])
    assert (cfg.eval_topk, cfg.eval_graph) == (3, False)


def test_train_reports_topk(monkeypatch, tmp_path):
    mags = []
    res = _train(monkeypatch, tmp_path, mags=mags)
    assert res.engine == "native" and len(res.history) == 2 and len(mags) == 2
    for h in res.history:
        assert h["val_samples"] == 6
        assert h["val_accuracy"] <= h["val_top5_accuracy"] <= 1.0
    # the host path (torch's CE on the fp32 logits): the same counts; each mean loss is within the plain
    # fp32 bound of the exact one -- per row 2^-20 (|lse| + |x_l|) <= 2^-20 (ln C + 2 max |x|), plus the
    # sum of six fp32 terms -- so the two differ by at most twice that
    host = _train(monkeypatch, tmp_path, eval_graph=False)
    for h, g, mag in zip(host.history, res.history, mags):
        assert h["val_accuracy"] == g["val_accuracy"] and h["val_top5_accuracy"] == g["val_top5_accuracy"]
        bound = 2 * (2.0 ** -20 * (math.log(CLASSES) + 2 * mag)
                     + (6 * 2.0 ** -24 + 2.0 ** -21) * max(h["val_loss"], g["val_loss"]))
        err = abs(h["val_loss"] - g["val_loss"])
        print(f"val_loss, host path against the pass: err / bound = {err / bound:.4f}")
        assert err <= bound, (h["val_loss"], g["val_loss"], bound)
    off = _train(monkeypatch, tmp_path, eval_topk=0)
    for h, g in zip(off.history, res.history):
        assert not any(k.startswith("val_top") for k in h)
        assert h["val_accuracy"] == g["val_accuracy"] and h["val_loss"] == g["val_loss"]
    three = _train(monkeypatch, tmp_path, eval_topk=3)
    for h, g in zip(three.history, res.history):
        assert "val_top5_accuracy" not in h
        assert g["val_accuracy"] <= h["val_top3_accuracy"] <= g["val_top5_accuracy"]


def test_train_reports_topk_frozen_backbone(monkeypatch, tmp_path):
    """The frozen-backbone runner feeds its logits to K.ce_eval: the record against float64 metrics of
    the same logits, taken from the runner right after the epoch's evaluation."""
    import numpy as np
    monkeypatch.setenv("DBX_MLRUNS", str(tmp_path / "mlruns"))
    monkeypatch.setenv("DBX_FORCE_CPU", "1")
    from dbx_distributed_pytorch_examples_amd.data.datasets import SyntheticImages
    from dbx_distributed_pytorch_examples_amd.models import FrozenBackboneClassifier
    from dbx_distributed_pytorch_examples_amd.train.engine import train
    tr_ds, ev_ds = SyntheticImages(8, SIZE, 3, CLASSES, seed=1), SyntheticImages(6, SIZE, 3, CLASSES, seed=2)
    img = torch.from_numpy(np.stack([ev_ds[i][0] for i in range(6)]))
    lab = torch.tensor([int(ev_ds[i][1]) for i in range(6)])
    want = []

    def oracle(epoch, rec, runner):
        tot = [0.0, 0.0, 0.0, 0.0]
        for lo, hi in ((0, N), (N, 6)):
            lg = runner.tr.evaluate_batch(img[lo:hi], lab[lo:hi])
            tot = [a + b for a, b in zip(tot, metrics64(lg, lab[lo:hi], 5))]
        want.append(tot)

    torch.manual_seed(0)
    res = train(_cfg(), model=FrozenBackboneClassifier("resnet18", num_classes=CLASSES), train_dataset=tr_ds,
                eval_dataset=ev_ds, log_mlflow=False, callbacks=[oracle])
    assert res.engine == "native" and len(res.history) == len(want) == 2
    for h, (loss, top1, top5, bound) in zip(res.history, want):
        assert (h["val_samples"], h["val_accuracy"], h["val_top5_accuracy"]) == (6, top1 / 6, top5 / 6)
        assert abs(h["val_loss"] - loss / 6) <= bound / 6, (h["val_loss"], loss / 6, bound / 6)


def test_train_reports_topk_autograd(monkeypatch, tmp_path):
    res = _train(monkeypatch, tmp_path, engine="autograd")
    assert res.engine == "autograd" and len(res.history) == 2
    for h in res.history:
        assert h["val_samples"] == 6 and h["val_loss"] > 0
        assert h["val_accuracy"] <= h["val_top5_accuracy"] <= 1.0
    off = _train(monkeypatch, tmp_path, engine="autograd", eval_topk=0)
    assert all(not any(k.startswith("val_top") for k in h) and "val_accuracy" in h for h in off.history)
