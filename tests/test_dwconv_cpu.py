"""Depthwise convolution on the CPU path: groups= on ops.conv2d and
layers.Conv2d against torch's own grouped convolution, the rejected cases,
and the MobileNet model built on it."""

import pytest
import torch

from mi355x import optim
from mi355x.models import build_model
from mi355x.models.layers import Conv2d
from mi355x.ops import cross_entropy
from mi355x.ops import functional as fn
from mi355x.parallel.flat import FlatState


def test_depthwise_module_matches_torch():
    torch.manual_seed(0)
    ref = torch.nn.Conv2d(16, 16, 3, 2, 1, groups=16)
    ours = Conv2d(16, 16, 3, 2, 1, groups=16)
    assert ours.weight.shape == ref.weight.shape == (16, 1, 3, 3)
    ours.load_state_dict(ref.state_dict())

    x_ref = torch.randn(3, 16, 9, 7, requires_grad=True)        # NCHW
    x_ours = x_ref.detach().permute(0, 2, 3, 1).contiguous()    # NHWC
    x_ours.requires_grad_(True)
    y_ref = ref(x_ref)
    y_ours = ours(x_ours)
    assert y_ours.shape == (3, 5, 4, 16)
    torch.testing.assert_close(y_ours.permute(0, 3, 1, 2), y_ref,
                               rtol=1e-5, atol=1e-6)

    dy = torch.randn_like(y_ref)
    y_ref.backward(dy)
    y_ours.backward(dy.permute(0, 2, 3, 1))
    torch.testing.assert_close(x_ours.grad.permute(0, 3, 1, 2), x_ref.grad,
                               rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(ours.weight.grad, ref.weight.grad,
                               rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(ours.bias.grad, ref.bias.grad,
                               rtol=1e-5, atol=1e-5)

    # and the other way round
    back = torch.nn.Conv2d(16, 16, 3, 2, 1, groups=16)
    back.load_state_dict(ours.state_dict())
    assert torch.equal(back.weight, ours.weight)
    assert torch.equal(back.bias, ours.bias)


def test_groups_one_is_todays_path():
    torch.manual_seed(1)
    w = torch.randn(8, 4, 3, 3)
    b = torch.randn(8)

    def run(**kw):
        x = torch.randn(2, 6, 6, 4, generator=torch.Generator().manual_seed(2))
        x.requires_grad_(True)
        wp, bp = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        y = fn.conv2d(x, wp, bp, 1, 1, "relu", **kw)
        y.square().sum().backward()
        return y.detach(), x.grad, wp.grad, bp.grad

    for got, want in zip(run(groups=1), run()):
        assert torch.equal(got, want)


@pytest.mark.parametrize("wshape,stride,pad,groups,names", [
    ((8, 4, 3, 3), 1, 1, 2, "groups=2"),          # general grouped conv
    ((16, 1, 3, 3), 1, 1, 8, r"got \(16, 1, 3, 3\)"),             # channel multiplier 2
    ((8, 1, 3, 5), 1, 1, 8, "3x5"),               # not square
    ((8, 1, 7, 7), 1, 3, 8, "7x7"),               # R = 7
    ((8, 1, 3, 3), 3, 1, 8, "stride .* got 3"),    # stride 3
    ((8, 1, 3, 3), 1, 3, 8, "padding .* got 3"),   # padding R
    ((8, 1, 5, 5), 1, 5, 8, "padding .* got 5"),   # padding R, 5x5
])
def test_rejected_cases_name_the_value(wshape, stride, pad, groups, names):
    x = torch.randn(1, 9, 9, 8)
    w = torch.randn(*wshape)
    with pytest.raises(ValueError, match=names):
        fn.conv2d(x, w, None, stride, pad, None, groups=groups)


def test_module_rejects_groups_that_do_not_divide():
    with pytest.raises(ValueError, match="groups=3"):
        Conv2d(8, 8, 3, groups=3)


def test_mobilenet_shapes_and_state_dict():
    torch.manual_seed(3)
    net = build_model("mobilenet")
    y = net(torch.randn(2, 3, 32, 32))
    assert y.shape == (2, 10)
    dw = [m for m in net.modules() if isinstance(m, Conv2d) and m.groups > 1]
    assert len(dw) == 12
    for m in dw:
        C = m.groups
        assert m.weight.shape == (C, 1, 3, 3)
    assert build_model("mobilenet", num_classes=7)(
        torch.randn(1, 3, 32, 32)).shape == (1, 7)

    other = build_model("mobilenet")
    other.load_state_dict(net.state_dict())
    net.eval(), other.eval()
    x = torch.randn(2, 3, 32, 32)
    assert torch.equal(other(x), net(x))


def test_mobilenet_trains_on_cpu():
    torch.manual_seed(4)
    net = build_model("mobilenet")
    flat = FlatState(net)
    opt = optim.SGD(flat, lr=0.05, momentum=0.9)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(8, 3, 32, 32, generator=g)
    y = torch.randint(0, 10, (8,), generator=g)
    losses = []
    for _ in range(4):
        opt.zero_grad()
        loss = cross_entropy(net(x), y)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert all(l == l for l in losses), losses
    assert losses[-1] < losses[0], losses
