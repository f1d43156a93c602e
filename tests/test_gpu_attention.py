"""csrc/attn.hip through ops.attention against the formula in float64 on the
same 16-bit inputs, with torch autograd.

Pass line per element of o and of dqkv: four times the worst absolute error
of an fp32 torch evaluation of that output against float64 (the rule of
tests/test_gpu_groupnorm.py), u16 * |ref| for the output's rounding, and the
operand roundings the kernel makes by design, from the float64 quantities:
o: u16 * (P |V|); dv: u16 * (P^T |dO|); dq: u16 * scale * (|dS| |K|);
dk: u16 * scale * (|dS|^T |Q|). Every case runs twice: the same bits.

Worst |kernel - ref| / bound over the cases, measured on an MI355X, is
recorded in profiles/r17_attention.md (at most 0.70 for o, 0.84 for dqkv).
"""

import pytest
import torch

import mi355x.ops as ops
from mi355x.ops import functional as fn
from _bn_pool_ref import u16

pytestmark = pytest.mark.gpu

BF, HF = torch.bfloat16, torch.float16

# (B, S, H, dh, dtype)
CASES = {
    "one-token": (2, 1, 1, 32, BF),
    "s31": (2, 31, 1, 32, BF),
    "s33-h3": (2, 33, 3, 64, BF),
    "model": (2, 64, 4, 64, BF),
    "s65": (2, 65, 2, 64, BF),
    "s197": (1, 197, 2, 64, BF),
    "s256-d64": (1, 256, 1, 64, BF),
    "s256-d32": (1, 256, 2, 32, BF),
    "model-fp16": (2, 64, 4, 64, HF),
    "dy-t": (2, 33, 2, 32, BF),      # non-contiguous dy
    "big-scores": (1, 33, 1, 64, BF),  # scale * q.k reaches about +-80
}


def _inputs(name):
    B, S, H, dh, dtype = CASES[name]
    g = torch.Generator().manual_seed(sorted(CASES).index(name))
    qkv = torch.randn(B, S, 3, H, dh, generator=g)
    if name == "big-scores":  # scale * q.k has sigma amp^2; the largest ~3.3
        qkv[:, :, :2] *= 80 ** 0.5 / 3.3 ** 0.5
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
    o = ops.attention(leaf, qkv.shape[3])
    return o.detach(), torch.autograd.grad(o, leaf, dy)[0]


def _torch_eval(work, qkv, dy):
    """o, dqkv in dtype `work`, and the design terms of the bound."""
    B, S, _, H, dh = qkv.shape
    scale = dh ** -0.5
    leaf = qkv.to(work).requires_grad_()
    q, k, v = (leaf[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    p = torch.softmax(scale * (q @ k.transpose(-1, -2)), dim=-1)
    o = (p @ v).permute(0, 2, 1, 3).reshape(B, S, H * dh)
    dqkv, = torch.autograd.grad(o, leaf, dy.to(work), retain_graph=True)
    with torch.no_grad():
        do = dy.to(work).reshape(B, S, H, dh).permute(0, 2, 1, 3)
        dp = do @ v.transpose(-1, -2)
        ds = (p * (dp - (p * dp).sum(-1, keepdim=True))).abs()
        back = lambda t: t.permute(0, 2, 1, 3)  # [B,H,S,dh] -> [B,S,H,dh]
        o_term = back(p @ v.abs()).reshape(B, S, H * dh)
        g_term = torch.stack(
            (back(scale * (ds @ k.abs())),
             back(scale * (ds.transpose(-1, -2) @ q.abs())),
             back(p.transpose(-1, -2) @ do.abs())), dim=2)
    return o.detach(), dqkv, o_term, g_term


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
    print(f"attn {name:12s} " + " ".join(f"{k}={r:.3f}"
                                         for k, r in worst.items()))
    assert all(r <= 1.0 for r in worst.values()), worst
    o2, dqkv2 = _kernel(qkv, dy)  # fixed order: the same bits
    assert torch.equal(o, o2) and torch.equal(dqkv, dqkv2)


@pytest.mark.parametrize("which", ("q", "k"))
def test_nan_placement(which):
    B, S, H, dh = 2, 33, 3, 64
    qkv = _inputs("s33-h3")[0].clone()
    b, s, h = 1, 20, 2
    qkv[b, s, 0 if which == "q" else 1, h, 5] = float("nan")
    with torch.no_grad():
        o = ops.attention(qkv, H).reshape(B, S, H, dh)
    bad = torch.zeros_like(o, dtype=torch.bool)
    if which == "q":
        bad[b, s, h] = True
    else:
        bad[b, :, h] = True
    assert torch.equal(torch.isnan(o), bad)


def test_captured_forward_backward_replays():
    """Capture form of tests/test_gpu_se.py; two replays against eager."""
    qkv, dy = _inputs("s33-h3")
    want = _kernel(qkv, dy)
    static = qkv.clone().requires_grad_()

    def step():
        static.grad = None
        o = ops.attention(static, 3)
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


def test_domain_errors_on_the_gpu():
    z = lambda *shape: torch.zeros(*shape, dtype=BF, device="cuda")
    with pytest.raises(ValueError, match="head width=48"):
        ops.attention(z(1, 8, 3, 2, 48), 2)
    with pytest.raises(ValueError, match="sequence length=257"):
        ops.attention(z(1, 257, 3 * 64), 1)
    with pytest.raises(ValueError, match="=200 is not divisible by .*=9"):
        ops.attention(z(1, 8, 200), 3)
    with pytest.raises(ValueError, match="float32"):
        fn._AttnFn.apply(z(1, 8, 3, 1, 32).float(), 32 ** -0.5)
