from .resnet import (BasicBlock, Bottleneck, ResNet, CifarBlock, CifarResNet18, build_model,
                     register_model, resnet18, resnet34, resnet50, resnet101, resnet152, SEModule, seresnet18, seresnet34,
                     seresnet50, seresnet101, seresnet152, seresnext50_32x4d, seresnext101_32x8d, BlurPool2d,
                     resnetblur18, resnetblur34, resnetblur50, resnetblur101, DropBlock2d)
from .mnist import Net
from .wrappers import ComposerResNet50, FrozenBackboneClassifier, resnet18_1ch

__all__ = [
    "BasicBlock", "Bottleneck", "ResNet", "CifarBlock", "CifarResNet18", "build_model",
    "register_model", "resnet18", "resnet34", "resnet50", "resnet101", "resnet152", "Net",
    "ComposerResNet50", "FrozenBackboneClassifier", "resnet18_1ch", "SEModule", "seresnet18", "seresnet34",
    "seresnet50", "seresnet101", "seresnet152", "seresnext50_32x4d", "seresnext101_32x8d",
    "BlurPool2d", "resnetblur18", "resnetblur34", "resnetblur50", "resnetblur101", "DropBlock2d",
]
