"""csrc/ln.hip through ops.layer_norm against float64 on the same 16-bit
inputs, by the convention of test_gpu_groupnorm.py.

Pass line, per case and output tensor: four times the worst absolute error
of an fp32 torch evaluation (nothing rounded to 16 bits) against the float64
reference, since the kernels sum in another order; the 16-bit outputs add
u16(dtype) * |ref| for their one rounding. s is checked against the float64
sum x + r; y and the gradients against float64 LayerNorm of the kernel's own
returned s.

Worst |kernel - ref| / bound over all cases, measured on an MI355X, is
recorded per output in profiles/r18_layernorm.md.
"""

import pytest
import torch
import torch.nn.functional as F

import mi355x.ops as ops
from _bn_pool_ref import u16

pytestmark = pytest.mark.gpu

BF, HF = torch.bfloat16, torch.float16
EPS = 1e-5

# (M, D, dtype, residual, ds, shift). A block is 4 waves of 64/L rows each.
CASES = {
    # L 4, 64 rows a block: the smallest row, 5 of a wave's 16 row slots used
    "d32-m5": (5, 32, BF, True, True, 0.0),
    # 4 and 10 partial rows (the few-rows and the sliced combine), the last
    # block holding one row
    "d32-parts4": (193, 32, BF, True, True, 0.0),
    "d32-parts10": (577, 32, BF, True, True, 0.0),
    # D/8 not a power of two: 4 lanes x 3 and 16 lanes x 3; ragged blocks
    "d96": (37, 96, BF, True, True, 0.0),
    "d384": (67, 384, BF, True, True, 0.0),
    # 64 lanes x 8: four masked trailing vectors, and full
    "d4064": (3, 4064, BF, True, True, 0.0),
    "d4096": (3, 4096, BF, True, True, 0.0),
    # the model's width, 32 lanes x 1, 8 rows a block, 17 blocks (2 rows last)
    "d256": (130, 256, BF, True, True, 0.0),
    "d256-nods": (130, 256, BF, True, False, 0.0),
    "d256-plain": (130, 256, BF, False, False, 0.0),
    "d256-fp16": (130, 256, HF, True, True, 0.0),
    # mean >> std: the variance must be centred
    "d256-shift": (130, 256, BF, True, True, 64.0),
    # every row constant: variance 0, rstd = eps ** -0.5, y == beta
    "d256-const": (10, 256, BF, False, False, 0.0),
}
NONCONTIG_DY = "d384"


def _inputs(name):
    M, D, dtype, has_res, has_ds, shift = CASES[name]
    g = torch.Generator().manual_seed(sorted(CASES).index(name))
    x = shift + torch.randn(M, D, generator=g)
    if name == "d256-const":
        x = (0.25 * torch.arange(M) - 1.0)[:, None].expand(M, D)
    x = x.to(dtype).cuda().contiguous()
    r = torch.randn(M, D, generator=g).to(dtype).cuda() if has_res else None
    gamma = 0.5 + torch.rand(D, generator=g)
    gamma[1], gamma[D - 2] = -0.7, -1.2
    beta = 0.3 * torch.randn(D, generator=g)
    dy = torch.randn(D, M, generator=g).to(dtype).cuda().t()
    if name != NONCONTIG_DY:
        dy = dy.contiguous()
    ds = torch.randn(M, D, generator=g).to(dtype).cuda() if has_ds else None
    return x, r, gamma.cuda(), beta.cuda(), dy, ds


def _kernel(x, r, gamma, beta, dy, ds):
    leaves = [t.clone().requires_grad_()
              for t in (x, gamma, beta) + ((r,) if r is not None else ())]
    if r is not None:
        s, y = ops.layer_norm(*leaves, EPS)
    else:  # s is x itself
        s, y = x, ops.layer_norm(*leaves, None, EPS)
    outs, douts = ((s, y), (ds, dy)) if ds is not None else ((y,), (dy,))
    grads = torch.autograd.grad(outs, leaves, douts)
    out = dict(s=s.detach(), y=y.detach(), dx=grads[0], dgamma=grads[1],
               dbeta=grads[2])
    if r is not None:
        out["dr"] = grads[3]
    return out


def _torch_eval(work, s_kernel, x, r, gamma, beta, dy, ds):
    """s = x + r, and LayerNorm of the kernel's s with the gradient of that
    s, in dtype `work`."""
    sd, gd, bd = (t.to(work).requires_grad_() for t in (s_kernel, gamma, beta))
    y = F.layer_norm(sd, sd.shape[-1:], gd, bd, EPS)
    d, dgamma, dbeta = torch.autograd.grad(y, (sd, gd, bd), dy.to(work))
    if ds is not None:
        d = d + ds.to(work)
    s = x.to(work) + r.to(work) if r is not None else x.to(work)
    return dict(s=s, y=y.detach(), dx=d, dr=d, dgamma=dgamma, dbeta=dbeta)


@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_backward_against_float64(name):
    dtype = CASES[name][2]
    inp = _inputs(name)
    got = _kernel(*inp)
    assert got["y"].dtype == dtype and got["dx"].dtype == dtype
    assert got["dgamma"].dtype == torch.float32
    ref = _torch_eval(torch.float64, got["s"], *inp)
    f32 = _torch_eval(torch.float32, got["s"], *inp)
    worst = {}
    for k, v in got.items():
        bound = 4 * (f32[k].double() - ref[k]).abs().max()
        if v.dtype == dtype:
            bound = bound + u16(dtype) * ref[k].abs()
        err = (v.double() - ref[k]).abs()
        worst[k] = float((err / bound.clamp_min(1e-300)).max())
    print(f"ln {name:12s} " + " ".join(f"{k}={r:.3f}"
                                       for k, r in worst.items()))
    assert all(r <= 1.0 for r in worst.values()), worst
    if "dr" in got:  # one tensor is both gradients of the add
        assert torch.equal(got["dr"], got["dx"])
    if name == "d256-const":
        assert all(bool(torch.isfinite(v).all()) for v in got.values())
        assert torch.equal(got["y"], inp[3].to(dtype).expand_as(got["y"]))
    again = _kernel(*inp)  # fixed-order reductions: the same bits
    assert all(torch.equal(got[k], again[k]) for k in got)


def test_captured_fused_forward_backward_replays():
    """Capture form of tests/test_gpu_mix.py; two replays against eager.
    Everything the op launches goes to the one capturing stream, so the
    captured graph is a single chain."""
    x, r, gamma, beta, dy, ds = _inputs("d384")
    dy = dy.contiguous()
    want = _kernel(x, r, gamma, beta, dy, ds)
    static = [t.clone().requires_grad_() for t in (x, gamma, beta, r)]

    def step():
        for t in static:
            t.grad = None
        s, y = ops.layer_norm(static[0], static[1], static[2], static[3], EPS)
        torch.autograd.backward((s, y), (ds, dy))
        return s, y

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s, y = step()
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        got = dict(s=s.detach(), y=y.detach(), dx=static[0].grad,
                   dgamma=static[1].grad, dbeta=static[2].grad,
                   dr=static[3].grad)
        assert all(torch.equal(got[k], want[k]) for k in want)


def test_other_dtypes_are_refused_on_the_gpu():
    w = torch.ones(64, device="cuda")
    with pytest.raises(ValueError, match="float32"):
        ops.layer_norm(torch.zeros(2, 64, device="cuda"), w, w)
