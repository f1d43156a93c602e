"""Depthwise convolution on the GPU: there is no kernel for it, and the op
says so instead of falling back to eager torch."""

import pytest
import torch

from mi355x.models import build_model
from mi355x.ops import functional as fn

pytestmark = pytest.mark.gpu


def test_depthwise_on_gpu_is_an_error_not_a_fallback():
    C = 16
    x = torch.randn(2, 6, 6, C, device="cuda").to(torch.bfloat16)
    w = torch.randn(C, 1, 3, 3, device="cuda")
    with pytest.raises(NotImplementedError, match="depthwise"):
        fn.conv2d(x, w, None, 1, 1, None, groups=C)
    # nothing was cast or cached for it
    assert not hasattr(w, "_mi355x_w16")


def test_domain_errors_come_first_on_gpu():
    x = torch.randn(2, 6, 6, 16, device="cuda").to(torch.bfloat16)
    with pytest.raises(ValueError, match="groups=2"):
        fn.conv2d(x, torch.randn(16, 8, 3, 3, device="cuda"), None, 1, 1,
                  None, groups=2)
    with pytest.raises(ValueError, match="7x7"):
        fn.conv2d(x, torch.randn(16, 1, 7, 7, device="cuda"), None, 1, 3,
                  None, groups=16)


def test_groups_one_on_gpu_is_todays_path():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 8, 8, 64, generator=g).cuda().to(torch.bfloat16)
    w = (torch.randn(64, 64, 3, 3, generator=g) * 0.2).cuda()
    assert torch.equal(fn.conv2d(x, w, None, 1, 1, "relu", groups=1),
                       fn.conv2d(x, w, None, 1, 1, "relu"))


def test_mobilenet_on_gpu_raises_at_its_first_depthwise_layer():
    net = build_model("mobilenet").cuda()
    with pytest.raises(NotImplementedError, match="depthwise"):
        net(torch.randn(2, 3, 32, 32, device="cuda"))
