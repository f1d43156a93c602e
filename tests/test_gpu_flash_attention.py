"""csrc/attn_flash.hip through ops.flash_attention against the formula in
float64 on the same 16-bit inputs, by the rule of tests/test_gpu_attention.py
(its _torch_eval and its bound: four times the fp32-torch error plus
u16 * (|ref| + the design terms)). The kernels round P, dS and each output
once, as attn.hip does, so the same terms apply; the online rescaling adds
fp32 roundings only. Every case runs twice: the same bits.

Worst |kernel - ref| / bound per case: profiles/r21_flash_attention.md.
"""

import pytest
import torch

import mi355x.ops as ops
from mi355x.models import layers
from mi355x.ops import functional as fn
from _bn_pool_ref import u16
from test_gpu_attention import _torch_eval

pytestmark = pytest.mark.gpu

BF, HF = torch.bfloat16, torch.float16

# (B, S, H, dh, dtype)
CASES = {
    "one-token": (2, 1, 1, 32, BF),
    "s63": (1, 63, 1, 64, BF),       # key-tile edges
    "s65": (1, 65, 2, 64, BF),
    "s129": (1, 129, 1, 32, BF),     # a block with one live query
    "s257": (1, 257, 2, 64, BF),     # first length past the resident kernels
    "s300-h3": (2, 300, 3, 32, BF),
    "s577": (1, 577, 2, 64, BF),     # ViT/16 at 384 px with a class token
    "s300-fp16": (1, 300, 2, 64, HF),
    "dy-t": (1, 300, 2, 32, BF),     # non-contiguous dy
    "big-scores": (1, 300, 1, 64, BF),  # scale * q.k reaches about +-80
    "rising-max": (1, 300, 1, 64, BF),  # every rescale has alpha < 1
}


def _inputs(name):
    B, S, H, dh, dtype = CASES[name]
    g = torch.Generator().manual_seed(sorted(CASES).index(name))
    qkv = torch.randn(B, S, 3, H, dh, generator=g)
    if name == "big-scores":  # as tests/test_gpu_attention.py scales them
        qkv[:, :, :2] *= 80 ** 0.5 / 3.3 ** 0.5
    if name == "rising-max":  # positive q and k, k row j times 1 + j / S
        qkv[:, :, :2] = qkv[:, :, :2].abs()
        qkv[:, :, 1] *= 1 + torch.arange(S).reshape(1, S, 1, 1) / S
    qkv = qkv.to(dtype).cuda()
    if name == "dy-t":
        dy = torch.randn(B, H * dh, S, generator=g).to(dtype).cuda()
        dy = dy.transpose(1, 2)
        assert not dy.is_contiguous()
    else:
        dy = torch.randn(B, S, H * dh, generator=g).to(dtype).cuda()
    return qkv, dy


def _kernel(qkv, dy):
    leaf = qkv.clone().requires_grad_()
    o = ops.flash_attention(leaf, qkv.shape[3])
    return o.detach(), torch.autograd.grad(o, leaf, dy)[0]


@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_backward_against_float64(name):
    dtype = CASES[name][4]
    qkv, dy = _inputs(name)
    o, dqkv = _kernel(qkv, dy)
    assert o.dtype == dtype and dqkv.dtype == dtype
    assert dqkv.shape == qkv.shape and dqkv.is_contiguous()
    assert not torch.isnan(o).any() and not torch.isnan(dqkv).any()
    ro, rg, o_term, g_term = _torch_eval(torch.float64, qkv, dy)
    fo, fg, _, _ = _torch_eval(torch.float32, qkv, dy)
    u = u16(dtype)
    worst = {}
    for key, got, ref, f32, term in (("o", o, ro, fo, o_term),
                                     ("dqkv", dqkv, rg, fg, g_term)):
        bound = 4 * (f32.double() - ref).abs().max() + u * (ref.abs() + term)
        err = (got.double() - ref).abs()
        worst[key] = float((err / bound.clamp_min(1e-300)).max())
    print(f"flash {name:12s} " + " ".join(f"{k}={r:.3f}"
                                          for k, r in worst.items()))
    assert all(r <= 1.0 for r in worst.values()), worst
    o2, dqkv2 = _kernel(qkv, dy)  # fixed order: the same bits
    assert torch.equal(o, o2) and torch.equal(dqkv, dqkv2)


@pytest.mark.parametrize("which", ("q", "k"))
def test_nan_placement(which):
    B, S, H, dh = CASES["s300-h3"][:4]
    qkv = _inputs("s300-h3")[0].clone()
    b, s, h = 1, 200, 2
    qkv[b, s, 0 if which == "q" else 1, h, 5] = float("nan")
    with torch.no_grad():
        o = ops.flash_attention(qkv, H).reshape(B, S, H, dh)
    bad = torch.zeros_like(o, dtype=torch.bool)
    if which == "q":
        bad[b, s, h] = True
    else:
        bad[b, :, h] = True
    assert torch.equal(torch.isnan(o), bad)


def test_captured_forward_backward_replays():
    """Capture form of tests/test_gpu_attention.py; two replays against
    eager."""
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(2, 300, 3, 2, 64, generator=g).to(BF).cuda()
    dy = torch.randn(2, 300, 128, generator=g).to(BF).cuda()
    want = _kernel(qkv, dy)
    static = qkv.clone().requires_grad_()

    def step():
        static.grad = None
        o = ops.flash_attention(static, 2)
        o.backward(dy)
        return o

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o = step()
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(o.detach(), want[0])
        assert torch.equal(static.grad, want[1])


def test_layer_past_256_tokens():
    torch.manual_seed(0)
    mha = layers.MultiHeadAttention(128, 2).cuda()
    x = torch.randn(2, 300, 128, device="cuda").to(BF).requires_grad_()
    y = mha(x)
    assert y.shape == x.shape
    y.float().sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all()
    assert all(p.grad is not None and p.grad.abs().sum() > 0
               for p in mha.parameters())


def test_domain_errors_on_the_gpu():
    z = lambda *shape: torch.zeros(*shape, dtype=BF, device="cuda")
    with pytest.raises(ValueError, match="sequence length=4097"):
        ops.flash_attention(z(1, 4097, 3 * 64), 1)
    with pytest.raises(ValueError, match="head width=48"):
        ops.flash_attention(z(1, 8, 3, 2, 48), 2)
    with pytest.raises(ValueError, match="float32"):
        fn._FlashAttnFn.apply(z(1, 8, 3, 1, 32).float(), 32 ** -0.5)
