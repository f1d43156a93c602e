"""Squeeze-and-excitation on the CPU path: ops.squeeze_excite against its
formulas written out in float64, the domain errors, the layer and the
SE-ResNet variant."""

import pytest
import torch

import mi355x.ops as ops
from mi355x.models import build_model
from mi355x.models.layers import SqueezeExcite


def se_formulas(x, w1, b1, w2, b2, res, relu):
    """The issue's four lines, in the dtype of the arguments."""
    s = x.mean(dim=(1, 2))
    z = torch.relu(s @ w1.t() + b1)
    g = torch.sigmoid(z @ w2.t() + b2)
    y = x * g[:, None, None, :]
    if res is not None:
        y = y + res
    return torch.relu(y) if relu else y


@pytest.mark.parametrize("has_res,act", [(True, "relu"), (False, "relu"),
                                         (True, None), (False, None)])
@pytest.mark.parametrize("C,Cr", [(64, 4), (8, 1), (96, 6)])
def test_op_matches_the_formulas_in_float64(C, Cr, has_res, act):
    g = torch.Generator().manual_seed(C + Cr)
    shapes = [(3, 5, 7, C), (Cr, C), (Cr,), (C, Cr), (C,), (3, 5, 7, C)]
    x, w1, b1, w2, b2, res = (torch.randn(*s, generator=g).requires_grad_()
                              for s in shapes)
    dy = torch.randn(3, 5, 7, C, generator=g)
    leaves = [x, w1, b1, w2, b2] + ([res] if has_res else [])
    got = ops.squeeze_excite(x, w1, b1, w2, b2, res if has_res else None, act)
    assert got.dtype == torch.float32
    got_g = torch.autograd.grad(got, leaves, dy)
    ref = [t.detach().double().requires_grad_() for t in leaves]
    want = se_formulas(*ref[:5], ref[5] if has_res else None, act == "relu")
    want_g = torch.autograd.grad(want, ref, dy.double())
    torch.testing.assert_close(got.double(), want, rtol=1e-5, atol=1e-5)
    for a, b in zip(got_g, want_g):
        torch.testing.assert_close(a.double(), b, rtol=1e-5, atol=1e-4)


def _args(C=64, Cr=4):
    return [torch.zeros(2, 4, 4, C), torch.zeros(Cr, C), torch.zeros(Cr),
            torch.zeros(C, Cr), torch.zeros(C)]


@pytest.mark.parametrize("change,says", [
    (lambda a: a.__setitem__(0, torch.zeros(4, 4, 64)), "3 dimensions"),
    (lambda a: a.__setitem__(0, torch.zeros(2, 4, 4, 12)), "channels=12"),
    (lambda a: a.__setitem__(0, torch.zeros(2, 2, 2, 2056)), "channels=2056"),
    (lambda a: a.__setitem__(1, torch.zeros(4, 32)), r"w1 .*\(4, 32\)"),
    (lambda a: (a.__setitem__(1, torch.zeros(257, 64)),
                a.__setitem__(2, torch.zeros(257)),
                a.__setitem__(3, torch.zeros(64, 257))),
     "reduced channels=257"),
    (lambda a: a.__setitem__(2, torch.zeros(5)), r"b1 .*\(5,\)"),
    (lambda a: a.__setitem__(3, torch.zeros(4, 64)), r"w2 .*\(4, 64\)"),
    (lambda a: a.__setitem__(4, torch.zeros(32)), r"b2 .*\(32,\)"),
    (lambda a: a.append(torch.zeros(2, 4, 4, 32)), r"residual \(2, 4, 4, 32\)"),
    (lambda a: a.append(torch.zeros(2, 4, 4, 64, dtype=torch.float64)),
     "residual .*float64"),
])
def test_domain_errors_name_the_value(change, says):
    args = _args()
    change(args)
    with pytest.raises(ValueError, match=says):
        ops.squeeze_excite(*args)


def test_layer_holds_two_linears():
    layer = SqueezeExcite(64, reduction=16, act="relu")
    shapes = {k: tuple(v.shape) for k, v in layer.state_dict().items()}
    assert shapes == {"fc1.weight": (4, 64), "fc1.bias": (4,),
                      "fc2.weight": (64, 4), "fc2.bias": (64,)}
    x, res = torch.randn(2, 3, 3, 64), torch.randn(2, 3, 3, 64)
    want = ops.squeeze_excite(x, layer.fc1.weight, layer.fc1.bias,
                              layer.fc2.weight, layer.fc2.bias, res, "relu")
    assert torch.equal(layer(x, residual=res), want)


def test_se_resnet18_trains_and_plain_keys_are_unchanged():
    torch.manual_seed(0)
    net = build_model("se_resnet18")
    out = net(torch.randn(2, 3, 32, 32))
    out.sum().backward()
    assert out.shape == (2, 10) and torch.isfinite(out).all()
    assert all(p.grad is not None and torch.isfinite(p.grad).all()
               for p in net.parameters())
    keys = set(build_model("resnet18").state_dict())
    assert len(keys) == 122  # as before this option existed
    blocks = [f"layer{i}.{j}" for i in (1, 2, 3, 4) for j in (0, 1)]
    se_keys = {f"{b}.se.{fc}.{p}" for b in blocks for fc in ("fc1", "fc2")
               for p in ("weight", "bias")}
    assert set(net.state_dict()) == keys | se_keys
    for name in ("se_resnet50", "se_resnet50_cifar"):
        assert sum(isinstance(m, SqueezeExcite)
                   for m in build_model(name).modules()) == 16
