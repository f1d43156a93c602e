from .mobilenet import MobileNet, mobilenet  # noqa: F401
from .net import Net  # noqa: F401
from .resnet import ResNet, resnet18, resnet50  # noqa: F401
from .vit import ViT, vit_cifar, vit_cifar_s, vit_s8  # noqa: F401


def build_model(name: str, num_classes: int = 10):
    name = name.lower()
    if name == "net":
        return Net()
    if name == "resnet18":
        return resnet18(num_classes=num_classes, stem="cifar")
    if name == "resnet18_imagenet":
        return resnet18(num_classes=num_classes, stem="imagenet")
    if name == "resnet50":
        return resnet50(num_classes=num_classes, stem="imagenet")
    if name == "resnet50_cifar":
        return resnet50(num_classes=num_classes, stem="cifar")
    if name == "resnet18_gn":
        return resnet18(num_classes=num_classes, stem="cifar", norm="gn")
    if name == "resnet50_gn":
        return resnet50(num_classes=num_classes, stem="imagenet", norm="gn")
    if name == "resnet50_cifar_gn":
        return resnet50(num_classes=num_classes, stem="cifar", norm="gn")
    if name == "se_resnet18":
        return resnet18(num_classes=num_classes, stem="cifar", se=16)
    if name == "se_resnet50":
        return resnet50(num_classes=num_classes, stem="imagenet", se=16)
    if name == "se_resnet50_cifar":
        return resnet50(num_classes=num_classes, stem="cifar", se=16)
    if name == "mobilenet":
        return mobilenet(num_classes=num_classes)
    if name == "vit_cifar":
        return vit_cifar(num_classes=num_classes)
    if name == "vit_cifar_s":
        return vit_cifar_s(num_classes=num_classes)
    if name == "vit_cifar_gelu":
        return vit_cifar(num_classes=num_classes, mlp_act="gelu")
    if name == "vit_cifar_s_gelu":
        return vit_cifar_s(num_classes=num_classes, mlp_act="gelu")
    if name == "vit_s8":
        return vit_s8(num_classes=num_classes)
    raise ValueError(f"unknown model {name!r}")
