"""MobileNet-v1 for 32-pixel input on the mi355x op layer.

Depthwise-separable blocks: a 3x3 depthwise convolution and a 1x1 pointwise
convolution, each followed by BN+ReLU. Every width is a multiple of 64, so
every pointwise convolution lands on the MFMA 1x1 kernels. The stem is the
CIFAR one of the ResNets (3x3/1, no pooling); the three stride-2 blocks
bring 32x32 down to 4x4 before the global average pool.

CPU only for now: ops.conv2d has no depthwise GPU kernel and raises
NotImplementedError for a depthwise layer on the GPU.
"""

from __future__ import annotations

from torch import nn

from .layers import BatchNorm2d, Conv2d, Linear, conv_bn, to_model_layout
from mi355x import ops

# (cin, cout, stride) of the depthwise-separable blocks, in order
BLOCKS = ((64, 128, 1), (128, 128, 1), (128, 256, 2), (256, 256, 1),
          (256, 512, 2), (512, 512, 1), (512, 512, 1), (512, 512, 1),
          (512, 512, 1), (512, 512, 1), (512, 1024, 2), (1024, 1024, 1))


class DWSeparable(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.dw = Conv2d(cin, cin, 3, stride, 1, bias=False, groups=cin)
        self.bn1 = BatchNorm2d(cin, act="relu")
        self.pw = Conv2d(cin, cout, 1, bias=False)
        self.bn2 = BatchNorm2d(cout, act="relu")

    def forward(self, x):
        x = conv_bn(self.dw, self.bn1, x)
        return conv_bn(self.pw, self.bn2, x)


class MobileNet(nn.Module):
    def __init__(self, num_classes=10):
        super().__init__()
        self.conv1 = Conv2d(3, 64, 3, 1, 1, bias=False)
        self.bn1 = BatchNorm2d(64, act="relu")
        self.blocks = nn.Sequential(*(DWSeparable(*b) for b in BLOCKS))
        self.fc = Linear(1024, num_classes)
        for m in self.modules():
            if isinstance(m, Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out",
                                        nonlinearity="relu")

    def forward(self, x):
        x = to_model_layout(x)  # NCHW -> NHWC, 16-bit on GPU
        x = conv_bn(self.conv1, self.bn1, x)
        x = self.blocks(x)
        x = ops.global_avg_pool(x)
        return self.fc(x)


def mobilenet(num_classes=10):
    return MobileNet(num_classes)
