"""ResNet-18/50 on the mi355x op layer (BASELINE configs 2-5).

Structure follows the standard He et al. residual nets; the hot path is
our NHWC HIP kernels with BN+ReLU (and BN+add+ReLU at block exits) fused
into single kernels. `stem="cifar"` (3x3/1 conv, no maxpool — the standard
CIFAR ResNet stem) for 32x32 inputs; `stem="imagenet"` (7x7/2 + maxpool
3x3/2) for 224x224 (BASELINE config 4).
"""

from __future__ import annotations

import torch
from torch import nn

from .layers import (BatchNorm2d, Conv2d, GroupNorm, Linear, MaxPool2d,
                     SqueezeExcite, _lazy_ok, bn_conv_lazy, bn_then_conv,
                     conv_bn, conv_bn_tap, conv_gn_tap, to_model_layout)
from mi355x import ops


def _norm(norm, gn_groups, channels, act=None):
    """The normalisation layer of a ResNet: "bn" BatchNorm2d, "gn" GroupNorm
    with gn_groups groups; the attribute names (bn1, ...) are shared."""
    if norm == "bn":
        return BatchNorm2d(channels, act=act)
    if norm == "gn":
        return GroupNorm(gn_groups, channels, act=act)
    raise ValueError(f"norm={norm!r}: expected 'bn' or 'gn'")


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, in_planes, planes, stride=1, downsample=None,
                 norm="bn", gn_groups=32, se=None):
        super().__init__()
        self.gn = norm == "gn"
        self.conv1 = Conv2d(in_planes, planes, 3, stride, 1, bias=False)
        self.bn1 = _norm(norm, gn_groups, planes, "relu")
        self.conv2 = Conv2d(planes, planes, 3, 1, 1, bias=False)
        # fused add+relu at exit: in bn2, or in the SE gate behind it
        self.bn2 = _norm(norm, gn_groups, planes, None if se else "relu")
        self.downsample = downsample
        self.se = SqueezeExcite(planes, se, act="relu") if se else None

    def forward(self, x):
        if self.se is not None:
            # the gate takes over bn2's residual add and ReLU; the TAP
            # shortcut stays, the lazy-BN path is not taken
            tap_fn = conv_gn_tap if self.gn else conv_bn_tap
            out, tap = tap_fn(self.conv1, self.bn1, x)
            identity = (tap if self.downsample is None
                        else self.downsample(tap))
            out = (self.bn2(self.conv2(out)) if self.gn
                   else conv_bn(self.conv2, self.bn2, out))
            return self.se(out, residual=identity)
        if self.gn:  # none of the BN-only fusions; the TAP shortcut stays
            out, tap = conv_gn_tap(self.conv1, self.bn1, x)
            identity = (tap if self.downsample is None
                        else self.downsample(tap))
            return self.bn2(self.conv2(out), residual=identity)
        # lazy-BN: bn1's apply fuses into conv2's A-loads (the normalized
        # activation never materializes); conv1 carries the junction-grad
        # TAP and emits bn1's stats from its epilogue
        if _lazy_ok(self.bn1, self.conv2, x) and x.requires_grad:
            from mi355x.ops import functional as F_

            y1, tap, stats1 = F_.conv2d_tap_stats(
                x, self.conv1.weight, self.conv1.stride, self.conv1.padding)
            identity = (tap if self.downsample is None
                        else self.downsample(tap))
            y2, stats2 = bn_conv_lazy(self.bn1, self.conv2, y1, stats1,
                                      want_stats=True)
            return self.bn2(y2, residual=identity, stats=stats2)
        # the shortcut consumes conv1's TAP: the junction gradient fuses
        # into conv1's dgrad epilogue (layers.conv_bn_tap) instead of
        # autograd adding two full tensors at the block input
        out, tap = conv_bn_tap(self.conv1, self.bn1, x)
        identity = tap if self.downsample is None else self.downsample(tap)
        out = conv_bn(self.conv2, self.bn2, out, residual=identity)
        return out


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, in_planes, planes, stride=1, downsample=None,
                 norm="bn", gn_groups=32, se=None):
        super().__init__()
        self.gn = norm == "gn"
        self.conv1 = Conv2d(in_planes, planes, 1, bias=False)
        self.bn1 = _norm(norm, gn_groups, planes, "relu")
        self.conv2 = Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = _norm(norm, gn_groups, planes, "relu")
        self.conv3 = Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = _norm(norm, gn_groups, planes * 4,
                         None if se else "relu")
        self.downsample = downsample
        self.se = (SqueezeExcite(planes * 4, se, act="relu") if se
                   else None)

    def forward(self, x):
        if self.se is not None:
            # the gate takes over bn3's residual add and ReLU; the TAP
            # shortcut stays, the lazy-BN path is not taken
            tap_fn = conv_gn_tap if self.gn else conv_bn_tap
            out, tap = tap_fn(self.conv1, self.bn1, x)
            identity = (tap if self.downsample is None
                        else self.downsample(tap))
            if self.gn:
                out = self.bn3(self.conv3(self.bn2(self.conv2(out))))
            else:
                out = conv_bn(self.conv2, self.bn2, out)
                out = conv_bn(self.conv3, self.bn3, out)
            return self.se(out, residual=identity)
        if self.gn:  # none of the BN-only fusions; the TAP shortcut stays
            out, tap = conv_gn_tap(self.conv1, self.bn1, x)
            identity = (tap if self.downsample is None
                        else self.downsample(tap))
            out = self.bn2(self.conv2(out))
            return self.bn3(self.conv3(out), residual=identity)
        # per-pair lazy dispatch: each internal BN fuses into its consumer
        # conv when eligible (bn_then_conv), else applies materialized —
        # one fused-stats chain either way
        if x.is_cuda and x.requires_grad and self.bn1.training and (
                _lazy_ok(self.bn1, self.conv2, x)
                or _lazy_ok(self.bn2, self.conv3, x)):
            from mi355x.ops import functional as F_

            y1, tap, stats1 = F_.conv2d_tap_stats(
                x, self.conv1.weight, self.conv1.stride, self.conv1.padding)
            identity = (tap if self.downsample is None
                        else self.downsample(tap))
            y2, stats2 = bn_then_conv(self.bn1, self.conv2, y1, stats1,
                                      want_stats=True)
            y3, stats3 = bn_then_conv(self.bn2, self.conv3, y2, stats2,
                                      want_stats=True)
            return self.bn3(y3, residual=identity, stats=stats3)
        out, tap = conv_bn_tap(self.conv1, self.bn1, x)
        identity = tap if self.downsample is None else self.downsample(tap)
        out = conv_bn(self.conv2, self.bn2, out)
        out = conv_bn(self.conv3, self.bn3, out, residual=identity)
        return out


class Downsample(nn.Module):
    def __init__(self, in_planes, out_planes, stride, norm="bn",
                 gn_groups=32):
        super().__init__()
        self.gn = norm == "gn"
        self.conv = Conv2d(in_planes, out_planes, 1, stride, bias=False)
        self.bn = _norm(norm, gn_groups, out_planes)

    def forward(self, x):
        if self.gn:
            return self.bn(self.conv(x))
        return conv_bn(self.conv, self.bn, x)


class ResNet(nn.Module):
    def __init__(self, block, layers, num_classes=10, stem="cifar",
                 norm="bn", gn_groups=32, se=None):
        super().__init__()
        self.in_planes = 64
        self.norm, self.gn_groups, self.se = norm, gn_groups, se
        if stem == "cifar":
            self.conv1 = Conv2d(3, 64, 3, 1, 1, bias=False)
            self.maxpool = None
        else:
            self.conv1 = Conv2d(3, 64, 7, 2, 3, bias=False)
            self.maxpool = MaxPool2d(3, 2, 1)
        self.bn1 = _norm(norm, gn_groups, 64, "relu")
        self.layer1 = self._make_layer(block, 64, layers[0], 1)
        self.layer2 = self._make_layer(block, 128, layers[1], 2)
        self.layer3 = self._make_layer(block, 256, layers[2], 2)
        self.layer4 = self._make_layer(block, 512, layers[3], 2)
        self.fc = Linear(512 * block.expansion, num_classes)
        for m in self.modules():
            if isinstance(m, Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out",
                                        nonlinearity="relu")

    def _make_layer(self, block, planes, blocks, stride):
        downsample = None
        if stride != 1 or self.in_planes != planes * block.expansion:
            downsample = Downsample(self.in_planes, planes * block.expansion,
                                    stride, self.norm, self.gn_groups)
        kw = dict(norm=self.norm, gn_groups=self.gn_groups, se=self.se)
        layers = [block(self.in_planes, planes, stride, downsample, **kw)]
        self.in_planes = planes * block.expansion
        layers += [block(self.in_planes, planes, **kw)
                   for _ in range(1, blocks)]
        return nn.Sequential(*layers)

    def forward(self, x):
        x = to_model_layout(x)  # NCHW -> NHWC, 16-bit on GPU
        if self.norm == "gn":
            x = self.bn1(self.conv1(x))
        else:
            x = conv_bn(self.conv1, self.bn1, x)
        if self.maxpool is not None:
            x = self.maxpool(x)
        x = self.layer1(x)
        x = self.layer2(x)
        x = self.layer3(x)
        x = self.layer4(x)
        x = ops.global_avg_pool(x)
        return self.fc(x)


def resnet18(num_classes=10, stem="cifar", norm="bn", gn_groups=32, se=None):
    """norm="gn": every BatchNorm2d becomes a GroupNorm(gn_groups) with the
    same activation (for small per-GPU batches, where batch statistics stop
    working). se=16: SE-ResNet (Hu et al. 2018), a SqueezeExcite gate with
    that reduction behind each block's last norm; the gate takes over the
    block's residual add and ReLU."""
    return ResNet(BasicBlock, [2, 2, 2, 2], num_classes, stem, norm,
                  gn_groups, se)


def resnet50(num_classes=1000, stem="imagenet", norm="bn", gn_groups=32,
             se=None):
    return ResNet(Bottleneck, [3, 4, 6, 3], num_classes, stem, norm,
                  gn_groups, se)
