"""ops.layer_norm on the CPU, layers.LayerNorm beyond powers of two, the
ViT forward with the adds fused into the norms, and vit_cifar_s."""

import pytest
import torch
import torch.nn.functional as F

import mi355x.ops as ops
from mi355x.models import build_model, layers


@pytest.mark.parametrize("D", (96, 384))
@pytest.mark.parametrize("fused", (False, True))
def test_cpu_op_against_float64(D, fused):
    g = torch.Generator().manual_seed(D + fused)
    x, r, dy, ds = (torch.randn(2, 5, D, generator=g) for _ in range(4))
    gamma, beta = torch.randn(D, generator=g), torch.randn(D, generator=g)
    leaves = [t.requires_grad_() for t in (x, gamma, beta, r)[:3 + fused]]
    l64 = [t.detach().double().requires_grad_() for t in leaves]
    if fused:  # (s, y), gradients into both
        got, dout = ops.layer_norm(x, gamma, beta, r), (ds, dy)
        s64 = l64[0] + l64[3]
        ref = (s64, F.layer_norm(s64, (D,), l64[1], l64[2], 1e-5))
    else:
        got, dout = (ops.layer_norm(x, gamma, beta),), (dy,)
        ref = (F.layer_norm(l64[0], (D,), l64[1], l64[2], 1e-5),)
    for a, b in zip(got, ref):
        assert a.dtype == torch.float32
        assert (a.double() - b).abs().max() < 1e-5
    grads = torch.autograd.grad(got, leaves, dout)
    refs = torch.autograd.grad(ref, l64, [t.double() for t in dout])
    for a, b in zip(grads, refs):
        assert (a.double() - b).abs().max() < 1e-4


def test_domain_errors():
    w = torch.ones(64)
    with pytest.raises(ValueError, match="D=48"):
        ops.layer_norm(torch.zeros(2, 48), torch.ones(48), torch.ones(48))
    with pytest.raises(ValueError, match="D=4128"):
        ops.layer_norm(torch.zeros(2, 4128), torch.ones(4128),
                       torch.ones(4128))
    with pytest.raises(ValueError, match=r"residual \(3, 64\)"):
        ops.layer_norm(torch.zeros(2, 64), w, w, torch.zeros(3, 64))
    with pytest.raises(ValueError, match=r"\[64\], got \(32,\)"):
        ops.layer_norm(torch.zeros(2, 64), torch.ones(32), w)


@pytest.mark.parametrize("dim", (384, 16))
def test_layer_matches_torch(dim):
    ours, theirs = layers.LayerNorm(dim), torch.nn.LayerNorm(dim)
    with torch.no_grad():
        theirs.weight.normal_()
        theirs.bias.normal_()
    ours.load_state_dict(theirs.state_dict())
    x, r = torch.randn(3, 5, dim), torch.randn(3, 5, dim)
    assert torch.allclose(ours(x), theirs(x), atol=1e-5)
    s, y = ours(x, r)
    assert torch.equal(s, x + r)
    assert torch.allclose(y, theirs(x + r), atol=1e-5)


def test_vit_cifar_s_forward_backward():
    torch.manual_seed(0)
    net = build_model("vit_cifar_s")
    assert net.dim == 384 and net.blocks[0].attn.num_heads == 6
    y = net(torch.randn(2, 3, 32, 32))
    assert y.shape == (2, 10)
    y.sum().backward()
    assert all(p.grad is not None and p.grad.abs().sum() > 0
               for p in net.parameters())


def test_vit_forward_equals_the_unfused_formula():
    torch.manual_seed(1)
    net = build_model("vit_cifar")
    img = torch.randn(2, 3, 32, 32)
    B, g, p = 2, net.grid, net.patch
    x = layers.to_model_layout(img).reshape(B, g, p, g, p, 3)
    x = net.embed(x.permute(0, 1, 3, 2, 4, 5).reshape(B * g * g, p * p * 3))
    x = x.reshape(B, g * g, net.dim) + net.pos
    s0, h0 = net.blocks[0](x)  # the stream and the MLP output, not yet added
    for i, b in enumerate(net.blocks):
        x = x + b.attn(b.norm1(x))
        h = b.fc2(b.fc1(b.norm2(x).reshape(-1, net.dim))).reshape(x.shape)
        if i == 0:
            assert torch.allclose(s0, x, atol=1e-5)
            assert torch.allclose(h0, h, atol=1e-5)
        x = x + h
    want = net.fc(ops.global_avg_pool(net.norm(x).reshape(B, g, g, net.dim)))
    assert torch.allclose(net(img), want, atol=1e-5, rtol=1e-5)
