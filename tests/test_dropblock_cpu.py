"""DropBlock off the GPU: the counter-based mask twin (ops/reference.py dropblock_mask), the model option and the
refusals."""
import math

import pytest
import torch
import torch.nn.functional as F

from dbx_distributed_pytorch_examples_amd.models import DropBlock2d, build_model
from dbx_distributed_pytorch_examples_amd.ops import kernels as K
from dbx_distributed_pytorch_examples_amd.ops import reference as R

cpu = torch.device("cpu")


def _dropped(N, H, W, C, p, block_size, seed=11, offset=2, site=1):
    bs, gamma = R.dropblock_geometry(H, W, block_size, p)
    bits, kept = R.dropblock_mask(N, H, W, C, R.dropblock_threshold(gamma), block_size, seed, offset, site)
    drop = 1.0 - R.dropblock_unpack(bits, C).permute(0, 3, 1, 2)
    assert kept == N * H * W * C - int(drop.sum())
    return drop, bs, gamma, bits


@pytest.mark.parametrize("shape,block_size,p", [((2, 7, 7, 64), 3, 0.2), ((1, 9, 6, 128), 5, 0.5),
                                                ((2, 16, 5, 64), 7, 0.3), ((3, 3, 3, 64), 3, 0.5)], ids=str)
def test_every_dropped_element_lies_in_a_dropped_window_inside_the_map(shape, block_size, p):
    drop, bs, _, _ = _dropped(*shape, p, block_size)
    assert bs % 2 == 1 and bs <= min(shape[1], shape[2]) and 0 < drop.sum() < drop.numel()
    centres = (F.avg_pool2d(drop, bs, 1, 0) == 1).float()  # windows inside the map only: no seed outside the interior
    assert torch.equal(F.max_pool2d(F.pad(centres, (bs // 2,) * 4), bs, 1, bs // 2), drop)


def test_seed_fraction_and_streams():
    N, H, W, C, p = 8, 8, 8, 128, 0.1  # block size 1: the dropped elements are the seeds, gamma = p
    drop, _, gamma, bits = _dropped(N, H, W, C, p, 1)
    n = drop.numel()
    assert gamma == p and abs(drop.sum().item() / n - gamma) < 5 * math.sqrt(gamma * (1 - gamma) / n)
    assert torch.equal(bits, _dropped(N, H, W, C, p, 1)[3])
    assert not torch.equal(bits, _dropped(N, H, W, C, p, 1, site=2)[3])
    assert not torch.equal(bits, _dropped(N, H, W, C, p, 1, offset=3)[3])


def test_model_option():
    plain, model = build_model("resnet50", 10), build_model("resnet50", 10, drop_block_rate=0.1)
    assert [n for n, _ in build_model("resnet50", 10, drop_block_rate=0.0).named_modules()] == \
        [n for n, _ in plain.named_modules()]
    assert list(model.state_dict()) == list(plain.state_dict())
    sites = [(n, m.block_size, m.gamma_scale, m.site) for n, m in model.named_modules() if isinstance(m, DropBlock2d)]
    assert [s[0] for s in sites] == [f"layer3.{i}.drop_block" for i in range(6)] + \
        [f"layer4.{i}.drop_block" for i in range(3)]
    assert {s[1:3] for s in sites[:6]} == {(5, 0.25)} and {s[1:3] for s in sites[6:]} == {(3, 1.0)}
    assert [s[3] for s in sites] == list(range(9))
    x = torch.randn(2, 64, 9, 9)
    drop = DropBlock2d(0.5, 3)
    assert torch.equal(drop.eval()(x), x) and not torch.equal(drop.train()(x), x)
    drop.philox = (5, 1, 0)  # the counter-based mask: the same call twice gives the same tensor
    assert torch.equal(drop(x), drop(x))


def test_refusals():
    from dbx_distributed_pytorch_examples_amd.config import TrainConfig, validate_train
    from dbx_distributed_pytorch_examples_amd.engine.native_module import native_module
    from dbx_distributed_pytorch_examples_amd.engine.native_trainer import NativeTrainer
    from dbx_distributed_pytorch_examples_amd.engine.program import ResNetProgram
    with pytest.raises(ValueError, match="drop_block_rate"):
        validate_train(TrainConfig(drop_block_rate=1.0))
    with pytest.raises(ValueError, match="drop_block_rate"):
        build_model("resnet18", 10, drop_block_rate=-0.1)
    with pytest.raises(ValueError, match="no DropBlock2d sites"):
        NativeTrainer(build_model("resnet18", 10), 2, (32, 32), cpu, use_graphs=False, drop_block_rate=0.1)
    with pytest.raises(ValueError, match="DropBlock2d"):
        native_module(build_model("resnet18", 10, drop_block_rate=0.1), 2, (32, 32), cpu)
    both = build_model("resnetblur18", 10, drop_block_rate=0.1)  # layer3.0 / layer4.0: a blur and a site in one block
    with pytest.raises(TypeError, match="both a BlurPool2d and a DropBlock2d"):
        ResNetProgram(both, 2, (64, 64), cpu)
    wide = build_model("resnet18", 10, drop_block_rate=0.1)
    wide.layer3[0].drop_block.block_size = 9
    with pytest.raises(TypeError, match="block size in 1..7"):
        ResNetProgram(wide, 2, (64, 64), cpu)
    assert not K.dropblock_supported(96, 7, 7, 3) and K.dropblock_supported(64, 7, 7, 7)
    bits, kept, one = torch.zeros(1, 4, 4, 2, dtype=torch.int32), torch.zeros(1, dtype=torch.int64), torch.ones(1)
    with pytest.raises(ValueError, match="block size in 1..7"):
        K.dropblock_mask(bits, kept, one.int(), one.int(), block_size=8, seed=1, site=0)
