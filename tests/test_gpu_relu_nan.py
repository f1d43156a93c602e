"""The fused ReLU epilogues keep a NaN (as torch.relu does) and are
otherwise max(v, 0): an overflow that became NaN in the forward pass has to
reach the gradient, where the loss scaler looks for it."""

import pytest
import torch

from mi355x import amp
from mi355x.ops import functional as fn

pytestmark = pytest.mark.gpu


def _check(y_relu, y_plain):
    """y_relu is the same kernel's output with the fused ReLU."""
    y_relu, y_plain = y_relu.float(), y_plain.float()
    nan = torch.isnan(y_plain)
    assert bool(nan.any()) and not bool(nan.all())
    assert torch.equal(torch.isnan(y_relu), nan)
    want = y_plain.clamp_min(0.0)
    assert bool((want[~nan] == 0).any()) and bool((want[~nan] > 0).any())
    assert torch.equal(y_relu[~nan], want[~nan])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("c,k,r,pad,hw", [(3, 6, 5, 0, 32),     # Net conv1
                                          (6, 16, 5, 0, 14),    # Net conv2
                                          (64, 64, 3, 1, 8),    # MFMA 3x3
                                          (64, 128, 1, 0, 8)])  # MFMA 1x1
def test_conv_relu_keeps_nan(dtype, c, k, r, pad, hw):
    g = torch.Generator().manual_seed(31)
    x = torch.randn(4, hw, hw, c, generator=g).cuda().to(dtype)
    w = (torch.randn(k, c, r, r, generator=g) * 0.2).cuda()
    b = torch.randn(k, generator=g).cuda()
    x[1, hw // 2, hw // 2, 0] = float("nan")
    with amp.autocast(dtype):
        y_plain = fn.conv2d(x, w, b, 1, pad, None)
        y_relu = fn.conv2d(x, w, b, 1, pad, "relu")
    _check(y_relu, y_plain)


@pytest.mark.parametrize("m,kk,n", [(16, 400, 120), (256, 512, 512)])
def test_linear_relu_keeps_nan(m, kk, n):
    g = torch.Generator().manual_seed(32)
    x = torch.randn(m, kk, generator=g).cuda().to(torch.bfloat16)
    w = (torch.randn(n, kk, generator=g) * 0.1).cuda()
    b = torch.randn(n, generator=g).cuda()
    x[m // 2, 3] = float("nan")
    _check(fn.linear(x, w, b, "relu"), fn.linear(x, w, b, None))


@pytest.mark.parametrize("c", [6, 64])       # generic and 8-wide kernels
def test_bn_relu_keeps_nan(c):
    g = torch.Generator().manual_seed(33)
    x = torch.randn(4, 8, 8, c, generator=g).cuda().to(torch.bfloat16)
    x[2, 3, 3, 1] = float("nan")
    gamma, beta = torch.ones(c).cuda(), torch.zeros(c).cuda()
    mean, var = torch.zeros(c).cuda(), torch.ones(c).cuda()
    y_plain = fn.batch_norm(x, gamma, beta, mean, var, False)
    y_relu = fn.batch_norm(x, gamma, beta, mean, var, False, act="relu")
    _check(y_relu, y_plain)

