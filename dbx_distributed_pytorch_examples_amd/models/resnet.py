"""ResNet family with torchvision-compatible parameter names.

The reference pulls its ResNets from torchvision (`models.resnet18/50`, e.g.
`/root/reference/01_torch_distributor/02_cifar_torch_distributor_resnet.py:141-159`,
`/root/reference/04_accelerate/01_cifar_accelerate.ipynb:475-479`,
`/root/reference/05_ray/02_cifar_resnet_pytorch_ray.ipynb:278-280`) and defines a
CIFAR-stem ResNet-18 in `/root/reference/setup/resnet18.py:3-67`. torchvision is not
available on this image, so the architectures are written here directly. State-dict
keys and parameter counts match torchvision exactly (tests/test_models.py pins
11,181,642 / 23,528,522 / 25,557,032 params; tests/test_resnext_cpu.py the ResNeXt and Wide ResNet
variants), so checkpoints move both ways.

Layout: these are ordinary ``nn.Module`` s (NCHW API, any device). On a GPU the
training engine (``dbx.engine``) re-plans them as NHWC bf16 programs that run the
hand-written HIP kernels in ``dbx.ops``; on CPU they run stock PyTorch ops. The
module tree is therefore the single source of truth for parameters/state dicts.
"""
from __future__ import annotations

import math
from typing import Callable, List, Optional, Sequence, Type, Union

import torch
import torch.nn as nn
import torch.nn.functional as F

__all__ = [
    "BasicBlock", "BlurPool2d", "Bottleneck", "DropBlock2d", "ResNet", "SEModule", "resnetblur18", "resnetblur34", "resnetblur50",
    "resnetblur101", "seresnet18", "seresnet34", "seresnet50", "seresnet101",
    "seresnet152", "seresnext50_32x4d", "seresnext101_32x8d", "resnet18", "resnet34", "resnet50",
    "resnet101", "resnet152", "resnext50_32x4d", "resnext101_32x8d", "resnext101_64x4d", "wide_resnet50_2",
    "wide_resnet101_2", "CifarBlock", "CifarResNet18", "build_model",
]


def conv3x3(cin: int, cout: int, stride: int = 1, groups: int = 1) -> nn.Conv2d:
    return nn.Conv2d(cin, cout, kernel_size=3, stride=stride, padding=1, groups=groups, bias=False)


def conv1x1(cin: int, cout: int, stride: int = 1) -> nn.Conv2d:
    return nn.Conv2d(cin, cout, kernel_size=1, stride=stride, bias=False)


class SEModule(nn.Module):
    """Squeeze-and-excitation gate (Hu et al. 2018) in timm's ``SEModule`` layout: ``fc1`` / ``fc2`` are 1x1 convs
    with a bias, the squeezed width is ``max(8, channels // reduction)``; returns ``x * sigmoid(fc2(relu(fc1(mean))))``."""

    def __init__(self, channels: int, reduction: int = 16):
        super().__init__()
        rd = max(8, channels // reduction)
        self.fc1 = nn.Conv2d(channels, rd, kernel_size=1, bias=True)
        self.fc2 = nn.Conv2d(rd, channels, kernel_size=1, bias=True)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        s = torch.sigmoid(self.fc2(F.relu(self.fc1(x.mean((2, 3), keepdim=True)))))
        return x * s


class BlurPool2d(nn.Module):
    """Anti-aliased down-sampling (Zhang 2019, "Making Convolutional Networks Shift-Invariant Again"; timm's
    ``BlurPool2d`` with filter size 3): reflect-pad by 1, then the depthwise filter ``[1,2,1] x [1,2,1] / 16`` at
    ``stride``. Output size ``(H - 1) // stride + 1``. No parameters and no persistent buffer, so a model's state
    dict does not know it is there."""

    def __init__(self, channels: int, stride: int = 2):
        super().__init__()
        self.channels, self.stride = channels, stride
        k = torch.tensor([1.0, 2.0, 1.0])
        self.register_buffer("filt", (k[:, None] * k[None, :] / 16.0)[None, None].repeat(channels, 1, 1, 1),
                             persistent=False)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), self.filt.to(x.dtype), stride=self.stride,
                        groups=self.channels)


class DropBlock2d(nn.Module):
    """DropBlock (Ghiasi et al. 2018) as timm's ``drop_block_2d`` with ``batchwise=False, with_noise=False``: in
    training, seeds are drawn per sample and channel with probability ``gamma`` inside the valid interior of the map,
    every ``bs x bs`` window around a seed is zeroed and the rest is scaled by ``numel / max(kept, 1)``; ``bs`` is
    ``block_size`` clipped to the map and made odd. The identity in evaluation. No parameters and no buffers.
    The seeds come from torch's generator, or -- when the attribute ``philox = (seed, offset, site)`` is set -- from
    the counter-based mask of the native step (``ops.reference.dropblock_mask``), element for element."""

    def __init__(self, drop_prob: float = 0.1, block_size: int = 7, gamma_scale: float = 1.0):
        super().__init__()
        if not 0.0 <= drop_prob < 1.0:
            raise ValueError(f"drop_prob must be in [0, 1), got {drop_prob}")
        if block_size < 1:
            raise ValueError(f"block_size must be at least 1, got {block_size}")
        self.drop_prob, self.block_size, self.gamma_scale = float(drop_prob), int(block_size), float(gamma_scale)
        self.philox = None

    def extra_repr(self) -> str:
        return f"drop_prob={self.drop_prob}, block_size={self.block_size}, gamma_scale={self.gamma_scale}"

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not self.training or self.drop_prob == 0.0:
            return x
        from ..ops import reference as R
        N, C, H, W = x.shape
        bs, gamma = R.dropblock_geometry(H, W, self.block_size, self.drop_prob, self.gamma_scale)
        if self.philox is not None:
            seed, offset, site = self.philox[:3]
            bits, kept = R.dropblock_mask(N, H, W, C, R.dropblock_threshold(gamma), bs, int(seed), int(offset), int(site))
            keep = R.dropblock_unpack(bits, C).permute(0, 3, 1, 2).to(x.device)
        else:
            r = bs // 2
            seeds = torch.zeros(N, C, H, W, device=x.device)
            seeds[:, :, r:H - r, r:W - r] = (torch.rand(N, C, H - 2 * r, W - 2 * r, device=x.device) < gamma).float()
            keep = 1.0 - F.max_pool2d(seeds, bs, 1, r)
            kept = int(keep.sum())
        return x * (keep * R.dropblock_scale(N * C * H * W, kept)).to(x.dtype)


class BasicBlock(nn.Module):
    """torchvision BasicBlock (two 3x3 convs), keys conv1/bn1/conv2/bn2/downsample.{0,1}. ``se_reduction`` > 0: an
    :class:`SEModule` ``se`` gates the output of bn2 before the shortcut add (timm's seresnet18 / 34).
    ``blur_pool`` (timm's resnetblur18): a stride-2 block runs conv1 at stride 1 and a :class:`BlurPool2d` ``blur``
    down-samples behind bn1 + ReLU; the shortcut is unchanged. ``drop_block_rate`` > 0: a :class:`DropBlock2d`
    ``drop_block`` of ``drop_block_size`` / ``drop_block_gamma`` sits behind bn1, in front of its ReLU (timm)."""

    expansion = 1

    def __init__(self, inplanes: int, planes: int, stride: int = 1,
                 downsample: Optional[nn.Module] = None, se_reduction: int = 0, blur_pool: bool = False,
                 drop_block_rate: float = 0.0, drop_block_size: int = 3, drop_block_gamma: float = 1.0):
        super().__init__()
        blur = blur_pool and stride == 2
        self.conv1 = conv3x3(inplanes, planes, 1 if blur else stride)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = conv3x3(planes, planes)
        self.bn2 = nn.BatchNorm2d(planes)
        if se_reduction > 0:  # (no attribute at all without it: the module tree and the RNG stream of before)
            self.se = SEModule(planes, se_reduction)
        if blur:  # (likewise)
            self.blur = BlurPool2d(planes, stride)
        if drop_block_rate > 0:  # (likewise)
            self.drop_block = DropBlock2d(drop_block_rate, drop_block_size, drop_block_gamma)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        identity = x
        out = self.bn1(self.conv1(x))
        drop = getattr(self, "drop_block", None)
        if drop is not None:
            out = drop(out)
        out = self.relu(out)
        blur = getattr(self, "blur", None)
        if blur is not None:
            out = blur(out)
        out = self.bn2(self.conv2(out))
        se = getattr(self, "se", None)
        if se is not None:
            out = se(out)
        if self.downsample is not None:
            identity = self.downsample(x)
        return self.relu(out + identity)


class Bottleneck(nn.Module):
    """torchvision v1.5 Bottleneck: stride lives on the 3x3 conv (SURVEY.md §2.4 note). ``groups`` / ``base_width``
    (ResNeXt, Wide ResNet): the inner width is ``int(planes * base_width / 64) * groups`` and the 3x3 conv is grouped.
    ``se_reduction`` > 0: an :class:`SEModule` ``se`` gates the output of bn3 before the shortcut add (SE-ResNet).
    ``blur_pool`` (timm's resnetblur50): a stride-2 block runs conv2 at stride 1 and a :class:`BlurPool2d` ``blur``
    down-samples behind bn2 + ReLU; the shortcut is unchanged. ``drop_block_rate`` > 0: a :class:`DropBlock2d`
    ``drop_block`` of ``drop_block_size`` / ``drop_block_gamma`` sits behind bn2, in front of its ReLU (timm)."""

    expansion = 4

    def __init__(self, inplanes: int, planes: int, stride: int = 1,
                 downsample: Optional[nn.Module] = None, groups: int = 1, base_width: int = 64,
                 se_reduction: int = 0, blur_pool: bool = False, drop_block_rate: float = 0.0,
                 drop_block_size: int = 3, drop_block_gamma: float = 1.0):
        super().__init__()
        width = int(planes * base_width / 64) * groups
        blur = blur_pool and stride == 2
        self.conv1 = conv1x1(inplanes, width)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = conv3x3(width, width, 1 if blur else stride, groups)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = conv1x1(width, planes * self.expansion)
        self.bn3 = nn.BatchNorm2d(planes * self.expansion)
        if se_reduction > 0:
            self.se = SEModule(planes * self.expansion, se_reduction)
        if blur:
            self.blur = BlurPool2d(width, stride)
        if drop_block_rate > 0:
            self.drop_block = DropBlock2d(drop_block_rate, drop_block_size, drop_block_gamma)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        drop = getattr(self, "drop_block", None)
        if drop is not None:
            out = drop(out)
        out = self.relu(out)
        blur = getattr(self, "blur", None)
        if blur is not None:
            out = blur(out)
        out = self.bn3(self.conv3(out))
        se = getattr(self, "se", None)
        if se is not None:
            out = se(out)
        if self.downsample is not None:
            identity = self.downsample(x)
        return self.relu(out + identity)


class ResNet(nn.Module):
    """torchvision-compatible ResNet.

    ``in_channels`` != 3 reproduces the Ray FashionMNIST variant that swaps conv1 for
    ``Conv2d(1, 64, 7, 2, 3)`` (`/root/reference/05_ray/01_fashion_mnist_pytorch_ray.ipynb:169-174`).
    ``groups`` / ``width_per_group`` (Bottleneck only): ResNeXt (32 x 4d, 32 x 8d, 64 x 4d) and Wide ResNet (1 x 128).
    ``se_reduction`` > 0: every block gets a squeeze-and-excitation gate of that reduction (SE-ResNet / SE-ResNeXt).
    ``blur_pool``: the anti-aliased ResNet (timm's resnetblurN) -- every stride-2 block down-samples with a
    :class:`BlurPool2d` behind its 3x3 conv, run at stride 1, and the stem pool becomes
    ``Sequential(MaxPool2d(3, 1, 1), BlurPool2d(64, 2))``. State-dict keys and parameter counts do not change.
    ``drop_block_rate`` > 0 (timm's argument of the same name): every block of layer3 gets a :class:`DropBlock2d`
    of block size 5 and gamma scale 0.25, every block of layer4 one of block size 3 and gamma scale 1.0; the sites
    are numbered in module order (``drop_block.site``). With rate 0 the module tree is what it was.
    """

    def __init__(self, block: Type[Union[BasicBlock, Bottleneck]], layers: Sequence[int],
                 num_classes: int = 1000, in_channels: int = 3,
                 zero_init_residual: bool = False, groups: int = 1, width_per_group: int = 64,
                 se_reduction: int = 0, blur_pool: bool = False, drop_block_rate: float = 0.0):
        super().__init__()
        if blur_pool:  # (no attribute without it)
            self.blur_pool = True
        if not 0.0 <= drop_block_rate < 1.0:
            raise ValueError(f"drop_block_rate must be in [0, 1), got {drop_block_rate}")
        if drop_block_rate > 0:  # (likewise)
            self.drop_block_rate = float(drop_block_rate)
        if se_reduction < 0:
            raise ValueError(f"se_reduction must be >= 0, got {se_reduction}")
        self.se_reduction = int(se_reduction)
        if (groups != 1 or width_per_group != 64) and block is not Bottleneck:
            raise ValueError("groups / width_per_group need the Bottleneck block")
        self.groups, self.base_width = groups, width_per_group
        self.block_type = block
        self.layers_cfg = list(layers)
        self.num_classes = num_classes
        self.inplanes = 64
        self.conv1 = nn.Conv2d(in_channels, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1) if not blur_pool else nn.Sequential(
            nn.MaxPool2d(kernel_size=3, stride=1, padding=1), BlurPool2d(64, stride=2))
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2)
        self.layer3 = self._make_layer(block, 256, layers[2], stride=2, drop_block=(5, 0.25))
        self.layer4 = self._make_layer(block, 512, layers[3], stride=2, drop_block=(3, 1.0))
        for site, mod in enumerate(m for m in self.modules() if isinstance(m, DropBlock2d)):
            mod.site = site
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(512 * block.expansion, num_classes)
        init_resnet_(self, zero_init_residual)

    def _make_layer(self, block, planes: int, blocks: int, stride: int = 1, drop_block=None) -> nn.Sequential:
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(
                conv1x1(self.inplanes, planes * block.expansion, stride),
                nn.BatchNorm2d(planes * block.expansion),
            )
        kw = dict(groups=self.groups, base_width=self.base_width) if block is Bottleneck else {}
        if self.se_reduction:
            kw["se_reduction"] = self.se_reduction
        if getattr(self, "blur_pool", False):
            kw["blur_pool"] = True
        if drop_block is not None and getattr(self, "drop_block_rate", 0.0) > 0:
            kw.update(drop_block_rate=self.drop_block_rate, drop_block_size=drop_block[0], drop_block_gamma=drop_block[1])
        layers: List[nn.Module] = [block(self.inplanes, planes, stride, downsample, **kw)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(self.inplanes, planes, **kw))
        return nn.Sequential(*layers)

    def forward_features(self, x: torch.Tensor) -> torch.Tensor:
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return torch.flatten(self.avgpool(x), 1)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.fc(self.forward_features(x))


def init_resnet_(model: nn.Module, zero_init_residual: bool = False) -> None:
    """torchvision initialisation: kaiming-normal(fan_out) convs, BN (1, 0), default Linear."""
    for m in model.modules():
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
        elif isinstance(m, (nn.BatchNorm2d, nn.GroupNorm)):
            nn.init.constant_(m.weight, 1)
            nn.init.constant_(m.bias, 0)
    if zero_init_residual:
        for m in model.modules():
            if isinstance(m, Bottleneck):
                nn.init.constant_(m.bn3.weight, 0)
            elif isinstance(m, BasicBlock):
                nn.init.constant_(m.bn2.weight, 0)


def resnet18(num_classes: int = 1000, **kw) -> ResNet:
    return ResNet(BasicBlock, [2, 2, 2, 2], num_classes=num_classes, **kw)


def resnet34(num_classes: int = 1000, **kw) -> ResNet:
    return ResNet(BasicBlock, [3, 4, 6, 3], num_classes=num_classes, **kw)


def resnet50(num_classes: int = 1000, **kw) -> ResNet:
    return ResNet(Bottleneck, [3, 4, 6, 3], num_classes=num_classes, **kw)


def resnet101(num_classes: int = 1000, **kw) -> ResNet:
    return ResNet(Bottleneck, [3, 4, 23, 3], num_classes=num_classes, **kw)


def resnet152(num_classes: int = 1000, **kw) -> ResNet:
    return ResNet(Bottleneck, [3, 8, 36, 3], num_classes=num_classes, **kw)


def resnext50_32x4d(num_classes: int = 1000, **kw) -> ResNet:
    return ResNet(Bottleneck, [3, 4, 6, 3], num_classes=num_classes, groups=32, width_per_group=4, **kw)


def resnext101_32x8d(num_classes: int = 1000, **kw) -> ResNet:
    return ResNet(Bottleneck, [3, 4, 23, 3], num_classes=num_classes, groups=32, width_per_group=8, **kw)


def resnext101_64x4d(num_classes: int = 1000, **kw) -> ResNet:
    return ResNet(Bottleneck, [3, 4, 23, 3], num_classes=num_classes, groups=64, width_per_group=4, **kw)


def wide_resnet50_2(num_classes: int = 1000, **kw) -> ResNet:
    return ResNet(Bottleneck, [3, 4, 6, 3], num_classes=num_classes, width_per_group=128, **kw)


def wide_resnet101_2(num_classes: int = 1000, **kw) -> ResNet:
    return ResNet(Bottleneck, [3, 4, 23, 3], num_classes=num_classes, width_per_group=128, **kw)


def _se(factory):
    return lambda num_classes=1000, **kw: factory(num_classes=num_classes, se_reduction=16, **kw)


# timm's seresnet* / seresnext*: every block gated, reduction 16
seresnet18, seresnet34, seresnet50 = _se(resnet18), _se(resnet34), _se(resnet50)
seresnet101, seresnet152 = _se(resnet101), _se(resnet152)
seresnext50_32x4d, seresnext101_32x8d = _se(resnext50_32x4d), _se(resnext101_32x8d)


def _blur(factory):
    return lambda num_classes=1000, **kw: factory(num_classes=num_classes, blur_pool=True, **kw)


# timm's resnetblur*: anti-aliased down-sampling in the stem and in every stride-2 block
resnetblur18, resnetblur34, resnetblur50, resnetblur101 = (_blur(resnet18), _blur(resnet34), _blur(resnet50),
                                                           _blur(resnet101))


# --------------------------------------------------------------------------------------
# CIFAR-stem ResNet-18 of /root/reference/setup/resnet18.py (keys: conv1, bn1,
# layer{1-4}.{0,1}.{conv1,bn1,conv2,bn2,skip_connection.{0,1}}, fc — SURVEY.md §5.4).
# --------------------------------------------------------------------------------------
class CifarBlock(nn.Module):
    """Residual block of `setup/resnet18.py:3-27` (skip = 1x1 conv + BN when shape changes)."""

    def __init__(self, cin: int, cout: int, stride: int = 1):
        super().__init__()
        self.conv1 = conv3x3(cin, cout, stride)
        self.bn1 = nn.BatchNorm2d(cout)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = conv3x3(cout, cout)
        self.bn2 = nn.BatchNorm2d(cout)
        self.skip_connection = nn.Sequential()
        if stride != 1 or cin != cout:
            self.skip_connection = nn.Sequential(conv1x1(cin, cout, stride), nn.BatchNorm2d(cout))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        return self.relu(out + self.skip_connection(x))


class CifarResNet18(nn.Module):
    """3x3-s1 stem + maxpool + 4x2 CifarBlocks + avgpool + fc (`setup/resnet18.py:29-67`)."""

    def __init__(self, num_classes: int = 10, in_channels: int = 3):
        super().__init__()
        self.num_classes = num_classes
        self.conv1 = nn.Conv2d(in_channels, 64, kernel_size=3, stride=1, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        cin = 64
        for i, (cout, stride) in enumerate([(64, 1), (128, 2), (256, 2), (512, 2)]):
            blocks = [CifarBlock(cin, cout, stride), CifarBlock(cout, cout, 1)]
            setattr(self, f"layer{i + 1}", nn.Sequential(*blocks))
            cin = cout
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(512, num_classes)

    def forward_features(self, x: torch.Tensor) -> torch.Tensor:
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return torch.flatten(self.avgpool(x), 1)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.fc(self.forward_features(x))


_FACTORIES: dict = {
    "resnet18": resnet18, "resnet34": resnet34, "resnet50": resnet50,
    "resnet101": resnet101, "resnet152": resnet152,
    "resnext50_32x4d": resnext50_32x4d, "resnext101_32x8d": resnext101_32x8d, "resnext101_64x4d": resnext101_64x4d,
    "wide_resnet50_2": wide_resnet50_2, "wide_resnet101_2": wide_resnet101_2,
    "seresnet18": seresnet18, "seresnet34": seresnet34, "seresnet50": seresnet50, "seresnet101": seresnet101,
    "seresnet152": seresnet152, "seresnext50_32x4d": seresnext50_32x4d, "seresnext101_32x8d": seresnext101_32x8d,
    "resnetblur18": resnetblur18, "resnetblur34": resnetblur34, "resnetblur50": resnetblur50,
    "resnetblur101": resnetblur101,
    "cifar_resnet18": lambda num_classes=10, **kw: CifarResNet18(num_classes, **kw),
}


def build_model(name: str, num_classes: int = 1000, **kw) -> nn.Module:
    """Factory used by configs/CLI: ``build_model("resnet50", 1000)``."""
    from . import mnist, wrappers  # noqa: F401  (register extra names)
    key = name.lower()
    if key not in _FACTORIES:
        raise KeyError(f"unknown model {name!r}; known: {sorted(_FACTORIES)}")
    m = _FACTORIES[key](num_classes=num_classes, **kw)
    # factory spec: lets checkpoint / MLflow loaders rebuild the module without unpickling code
    m._dbx_spec = {"name": key, "kwargs": dict(num_classes=num_classes, **{k: v for k, v in kw.items()
                                                                          if isinstance(v, (int, float, str, bool))})}
    return m


def register_model(name: str, factory: Callable[..., nn.Module]) -> None:
    _FACTORIES[name.lower()] = factory
