"""ResNeXt (grouped conv2) and Wide ResNet bottlenecks through the native program, against fp32 autograd."""
import copy

import pytest
import torch
import torch.nn.functional as F

from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer, OptimConfig
from dbx_distributed_pytorch_examples_amd.models.resnet import Bottleneck, ResNet

pytestmark = pytest.mark.gpu
dev = torch.device("cuda")
SIZE, BATCH = 64, 8


def _model(groups, width):
    # widths 128 .. 1024: groups=32 gives cpg 4, 8, 16, 32 and all three stride-2 grouped convs
    torch.manual_seed(0)
    model = ResNet(Bottleneck, [1, 1, 1, 1], num_classes=100, groups=groups, width_per_group=width)
    for n, m in model.named_modules():
        if n.endswith("bn3"):  # damped residual branches, as test_program_matches_autograd
            torch.nn.init.constant_(m.weight, 0.2)
    return model


def _batch():
    g = torch.Generator().manual_seed(1)
    return (torch.randint(0, 256, (BATCH, SIZE, SIZE, 3), dtype=torch.uint8, generator=g).to(dev),
            torch.randint(0, 100, (BATCH,), generator=g).to(dev))


def _cos(a, b):
    a, b = a.float().flatten(), b.float().flatten()
    return (a @ b / (a.norm() * b.norm() + 1e-20)).item()


@pytest.mark.parametrize("groups,width", [(32, 4), (1, 128)], ids=["resnext", "wide"])
def test_program_matches_autograd(groups, width):
    model = _model(groups, width)
    ref = copy.deepcopy(model).to(dev).train()
    tr = NativeTrainer(model, BATCH, (SIZE, SIZE), dev, optim=OptimConfig(lr=0.0, momentum=0.0, weight_decay=0.0),
                       use_graphs=False)
    p = tr.prog
    img, lab = _batch()
    tr.step(img, lab)
    torch.cuda.synchronize()
    loss_native = p.metrics[0].item() / BATCH
    loss = F.cross_entropy(ref(p.x4[..., :3].float().permute(0, 3, 1, 2).contiguous()), lab)
    loss.backward()
    assert abs(loss_native - loss.item()) / loss.item() < 3e-2, (loss_native, loss.item())
    named_ref = dict(ref.named_parameters())
    for name, prm in model.named_parameters():
        off = (prm.data_ptr() - p.master.data_ptr()) // 4
        gflat = p.grad[off:off + prm.numel()]
        gn = (gflat.view(prm.shape[0], prm.shape[2], prm.shape[3], prm.shape[1]).permute(0, 3, 1, 2)
              if prm.dim() == 4 else gflat.view(prm.shape))
        c = _cos(gn, named_ref[name].grad)
        assert c > (0.9 if prm.dim() > 1 else 0.75), (name, c)


def test_graph_replay_matches_eager():
    m1 = _model(32, 4)
    m2 = copy.deepcopy(m1)
    t1 = NativeTrainer(m1, BATCH, (SIZE, SIZE), dev, optim=OptimConfig(lr=0.05), use_graphs=True)
    t2 = NativeTrainer(m2, BATCH, (SIZE, SIZE), dev, optim=OptimConfig(lr=0.05), use_graphs=False)
    img, lab = _batch()
    for i in range(5):
        t1.step(img, lab)
        t2.step(img, lab)
        assert t1.read_metrics()[0] == t2.read_metrics()[0], i
    assert torch.equal(t1.prog.master, t2.prog.master)
