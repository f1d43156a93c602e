"""ops.flash_attention on the CPU, the layer past 256 tokens, a 1024-token
ViT and vit_s8. Tolerances are those of tests/test_attention_cpu.py."""

import pytest
import torch

import mi355x.ops as ops
from mi355x.models import ViT, build_model, layers
from mi355x.ops import functional as fn
from test_attention_cpu import _ref64


@pytest.mark.parametrize("shape,H", (((1, 300, 3 * 2 * 32), 2),
                                     ((1, 300, 3, 1, 64), 1)))
def test_cpu_op_against_float64(shape, H):
    qkv = torch.randn(*shape, generator=torch.Generator().manual_seed(0))
    qkv.requires_grad_()
    o = ops.flash_attention(qkv, H)
    ref = _ref64(qkv, H)
    assert o.shape == ref.shape and o.dtype == torch.float32
    assert (o.double() - ref).abs().max() < 1e-5
    dy = torch.randn(*o.shape, generator=torch.Generator().manual_seed(1))
    g, = torch.autograd.grad(o, qkv, dy)
    g64, = torch.autograd.grad(ref, qkv, dy.double())
    assert (g - g64).abs().max() < 1e-4


def test_domain_errors():
    with pytest.raises(ValueError, match="sequence length=4097"):
        ops.flash_attention(torch.zeros(1, 4097, 3 * 64), 1)
    with pytest.raises(ValueError, match="head width=48"):
        ops.flash_attention(torch.zeros(1, 8, 3, 2, 48), 2)
    with pytest.raises(ValueError, match="float32"):
        fn._FlashAttnFn.apply(torch.zeros(1, 8, 3, 1, 32), 32 ** -0.5)


def test_layer_past_256_tokens():
    torch.manual_seed(0)
    mha = layers.MultiHeadAttention(64, 2)
    x = torch.randn(1, 300, 64, requires_grad=True)
    y = mha(x)
    assert y.shape == x.shape
    y.sum().backward()
    assert torch.isfinite(x.grad).all() and x.grad.abs().sum() > 0


def test_vit_1024_tokens_forward_backward():
    torch.manual_seed(0)
    net = ViT(image=32, patch=1, dim=64, depth=1, heads=2, mlp_dim=64)
    y = net(torch.randn(1, 3, 32, 32))
    assert y.shape == (1, 10)
    y.sum().backward()
    assert all(p.grad is not None and p.grad.abs().sum() > 0
               for p in net.parameters())


def test_vit_s8_state_dict_round_trip():
    net = build_model("vit_s8")
    assert net.pos.shape == (784, 384) and len(net.blocks) == 12
    twin = build_model("vit_s8")
    twin.load_state_dict(net.state_dict())
    assert all(torch.equal(a, b) for a, b in
               zip(net.state_dict().values(), twin.state_dict().values()))
