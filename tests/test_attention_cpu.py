"""ops.attention on the CPU, layers.LayerNorm and the vit_cifar model."""

import pytest
import torch

import mi355x.ops as ops
from mi355x.models import build_model, layers


def _ref64(qkv, H):
    B, S = qkv.shape[:2]
    q, k, v = (qkv.double().reshape(B, S, 3, H, -1)[:, :, i].transpose(1, 2)
               for i in range(3))
    p = torch.softmax(q @ k.transpose(-1, -2) * q.shape[-1] ** -0.5, dim=-1)
    return (p @ v).transpose(1, 2).reshape(B, S, -1)


@pytest.mark.parametrize("shape,H", (((2, 33, 3 * 2 * 32), 2),
                                     ((1, 64, 3, 4, 64), 4)))
def test_cpu_op_against_float64(shape, H):
    qkv = torch.randn(*shape, generator=torch.Generator().manual_seed(0))
    qkv.requires_grad_()
    o = ops.attention(qkv, H)
    ref = _ref64(qkv, H)
    assert o.shape == ref.shape and o.dtype == torch.float32
    assert (o.double() - ref).abs().max() < 1e-5
    dy = torch.randn(*o.shape, generator=torch.Generator().manual_seed(1))
    g, = torch.autograd.grad(o, qkv, dy)
    g64, = torch.autograd.grad(ref, qkv, dy.double())
    assert (g - g64).abs().max() < 1e-4


def test_domain_errors():
    with pytest.raises(ValueError, match="head width=48"):
        ops.attention(torch.zeros(1, 8, 3, 2, 48), 2)
    with pytest.raises(ValueError, match="sequence length=257"):
        ops.attention(torch.zeros(1, 257, 3 * 64), 1)
    with pytest.raises(ValueError, match="=200 is not divisible by .*=9"):
        ops.attention(torch.zeros(1, 8, 200), 3)
    with pytest.raises(ValueError, match="scale=-1.0"):
        ops.attention(torch.zeros(1, 8, 96), 1, scale=-1.0)
    with pytest.raises(ValueError, match="dim=48"):
        layers.LayerNorm(48)


def test_layer_norm_matches_torch():
    ours, theirs = layers.LayerNorm(64), torch.nn.LayerNorm(64)
    with torch.no_grad():
        theirs.weight.normal_()
        theirs.bias.normal_()
    ours.load_state_dict(theirs.state_dict())
    x = torch.randn(3, 5, 64)
    assert torch.allclose(ours(x), theirs(x), atol=1e-5)


def test_vit_cifar_forward_backward_state_dict():
    torch.manual_seed(0)
    net = build_model("vit_cifar")
    y = net(torch.randn(2, 3, 32, 32))
    assert y.shape == (2, 10)
    y.sum().backward()
    assert all(p.grad is not None and p.grad.abs().sum() > 0
               for p in net.parameters())
    twin = build_model("vit_cifar")
    twin.load_state_dict(net.state_dict())
    assert all(torch.equal(a, b) for a, b in
               zip(net.state_dict().values(), twin.state_dict().values()))
