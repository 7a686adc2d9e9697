"""DropBlock through the native program on the GPU: against fp32 autograd whose DropBlock2d modules draw the program's
Philox masks, with the damping and the criteria of tests/test_program_gpu.py::test_program_matches_autograd (and
evaluation against the same model without sites); captured against eager with a fresh mask per replay; a changed rate;
training; the refused combination."""
import copy

import pytest
import torch
import torch.nn.functional as F
from test_se_program_gpu import _batch, _cos, _trainer

from dbx_distributed_pytorch_examples_amd.engine.native_trainer import OptimConfig
from dbx_distributed_pytorch_examples_amd.models import Bottleneck, DropBlock2d, ResNet, build_model

pytestmark = pytest.mark.gpu
dev = torch.device("cuda")


def _model(arch, classes=100, rate=0.2):
    torch.manual_seed(0)
    m = (ResNet(Bottleneck, [1, 1, 1, 1], num_classes=classes, drop_block_rate=rate) if arch == "bottleneck"
         else build_model(arch, num_classes=classes, drop_block_rate=rate))
    for n_, m_ in m.named_modules():  # test_program_matches_autograd's damping: last-BN gamma = 0.2
        if n_.endswith("bn3") or (n_.endswith("bn2") and "layer" in n_ and "18" in arch):
            torch.nn.init.constant_(m_.weight, 0.2)
    return m


@pytest.mark.parametrize("arch,size", [("bottleneck", 128), ("resnet18", 64)])
def test_dropblock_program_matches_autograd(arch, size):
    model = _model(arch)
    ref = copy.deepcopy(model).to(dev).train()
    tr = _trainer(model, 8, size, seed=5)
    p = tr.prog
    img, lab = _batch(8, size, p.num_classes)
    tr.step(img, lab)
    torch.cuda.synchronize()
    state = tr.last_drop_block
    assert len(state) == len(p.db_blocks) > 1 and any(s["kept"] < s["numel"] for s in state), state
    for m_ in ref.modules():  # the program's masks: its seed, the offset the step used, the site's index
        if isinstance(m_, DropBlock2d):
            m_.philox = (p.db_seed, p.db_off.item(), m_.site)
    loss_native = p.metrics[0].item() / 8
    logits = ref(p.x4[..., :3].float().permute(0, 3, 1, 2).contiguous())
    loss = F.cross_entropy(logits, lab)
    loss.backward()
    print(arch, "loss", loss_native, loss.item(), "logits", _cos(p.logits, logits), state)
    assert abs(loss_native - loss.item()) / loss.item() < 3e-2 and _cos(p.logits, logits) > 0.98
    named_ref = dict(ref.named_parameters())
    for name, prm in model.named_parameters():
        off = (prm.data_ptr() - p.master.data_ptr()) // 4
        gflat = p.grad[off:off + prm.numel()]
        gn = (gflat.view(prm.shape[0], prm.shape[2], prm.shape[3], prm.shape[1]).permute(0, 3, 1, 2) if prm.dim() == 4
              else gflat.view(prm.shape))
        c = _cos(gn, named_ref[name].grad)
        assert c > (0.9 if prm.dim() > 1 else 0.75), (name, c)
    # evaluation applies nothing: the model without sites, the same weights and running statistics (lr = 0)
    out = tr.evaluate_batch(img, lab).float()
    plain = _model(arch, rate=0.0).to(dev)
    plain.load_state_dict(model.state_dict())
    with torch.no_grad():
        want = plain.eval()(p.x4[..., :3].float().permute(0, 3, 1, 2).contiguous())
    assert _cos(out, want) > 0.98, _cos(out, want)


def test_captured_equals_eager_with_a_fresh_mask_per_replay():
    opt = OptimConfig(lr=0.05, momentum=0.9, weight_decay=1e-4)
    a, b = (_trainer(_model("bottleneck"), 8, 128, optim=opt, seed=5, use_graphs=g) for g in (False, True))
    kept = []
    for i in range(3):
        img, lab = _batch(8, 128, 100, seed=10 + i)
        a.step(img, lab)
        b.step(img, lab)
        torch.cuda.synchronize()
        assert torch.equal(a.prog.grad, b.prog.grad) and torch.equal(a.prog.master, b.prog.master), i
        assert a.last_drop_block == b.last_drop_block
        kept.append(tuple(s["kept"] for s in b.last_drop_block))
    assert len(set(kept)) == 3, kept
    # a new rate reaches the next replay through the threshold table: p = 0 keeps everything
    b.set_drop_block_rate(0.0)
    b.step(img, lab)
    assert all(s["kept"] == s["numel"] and s["scale"] == 1.0 for s in b.last_drop_block), b.last_drop_block
    b.set_drop_block_rate(0.5)
    b.step(img, lab)
    assert all(s["kept"] < k for s, k in zip(b.last_drop_block, kept[-1])), (b.last_drop_block, kept)


def test_sgd_learns_and_the_blur_block_is_refused():
    with pytest.raises(TypeError, match="both a BlurPool2d and a DropBlock2d"):
        _trainer(build_model("resnetblur18", num_classes=4, drop_block_rate=0.1), 16, 64)
    # a learnable synthetic task: the label is the brightest image quadrant
    tr = _trainer(_model("resnet18", classes=4, rate=0.1), 16, 64, optim=OptimConfig(lr=0.05, momentum=0.9))
    g = torch.Generator().manual_seed(3)
    losses = []
    for _ in range(20):
        lab = torch.randint(0, 4, (16,), generator=g)
        img = torch.randint(0, 96, (16, 64, 64, 3), dtype=torch.uint8, generator=g)
        for n, q in enumerate(lab.tolist()):
            img[n, (q // 2) * 32:(q // 2) * 32 + 32, (q % 2) * 32:(q % 2) * 32 + 32] += 128
        tr.step(img.to(dev), lab.to(dev))
        losses.append(tr.read_metrics()[0] / 16)
    assert torch.isfinite(tr.prog.master).all() and sum(losses[-3:]) < 0.7 * sum(losses[:3]), losses
