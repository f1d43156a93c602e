"""ops.mlp on the CPU: the torch composition, the domain errors, layers.MLP
and the GELU ViT's checkpoint compatibility with vit_cifar."""

import pytest
import torch
import torch.nn.functional as F

import mi355x.ops as ops
from mi355x.models import build_model
from mi355x.models.layers import MLP


def _params(D=16, Fh=24):
    g = torch.Generator().manual_seed(0)
    shapes = ((5, D), (Fh, D), (Fh,), (D, Fh), (D,))
    return [torch.randn(*s, generator=g).requires_grad_() for s in shapes]


@pytest.mark.parametrize("act", ("gelu", "relu"))
def test_cpu_path_is_the_torch_composition(act):
    x, w1, b1, w2, b2 = _params()
    fa = F.gelu if act == "gelu" else F.relu
    want = F.linear(fa(F.linear(x, w1, b1)), w2, b2)
    got = ops.mlp(x, w1, b1, w2, b2, act=act)
    assert torch.equal(got, want)
    dy = torch.randn_like(want)
    leaves = (x, w1, b1, w2, b2)
    for a, b in zip(torch.autograd.grad(got, leaves, dy),
                    torch.autograd.grad(want, leaves, dy)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("change, match", [
    (dict(D=12), "D=12"),
    (dict(Fh=20), "F=20"),
    (dict(w2=torch.zeros(16, 16)), r"w2 must be \[16, 24\], got \(16, 16\)"),
    (dict(b1=None), "b1=None"),
    (dict(act="tanh"), "act='tanh'"),
])
def test_domain_errors_name_the_value(change, match):
    sizes = {k: change[k] for k in ("D", "Fh") if k in change}
    x, w1, b1, w2, b2 = _params(**sizes)
    args = dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2, act="gelu")
    args.update({k: v for k, v in change.items() if k in args})
    with pytest.raises(ValueError, match=match):
        ops.mlp(**args)


def test_mlp_layer_state_dict_keys():
    layer = MLP(16, 32)
    assert list(layer.state_dict()) == ["fc1.weight", "fc1.bias",
                                        "fc2.weight", "fc2.bias"]
    assert layer(torch.randn(3, 16)).shape == (3, 16)


def test_gelu_vit_loads_a_vit_cifar_checkpoint_and_trains():
    torch.manual_seed(0)
    net = build_model("vit_cifar_gelu")
    res = net.load_state_dict(build_model("vit_cifar").state_dict())
    assert not res.missing_keys and not res.unexpected_keys
    opt = torch.optim.SGD(net.parameters(), lr=0.01)
    loss = ops.cross_entropy(net(torch.randn(2, 3, 32, 32)),
                             torch.tensor([1, 7]))
    loss.backward()
    opt.step()
    assert torch.isfinite(loss)
    assert all(p.grad is not None for p in net.parameters())
