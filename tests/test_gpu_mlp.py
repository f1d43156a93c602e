"""csrc/mlp.hip through ops.mlp against the formula in float64 on the same
16-bit inputs (parameters included), with torch autograd and a random dy.

Pass line per element (the rule of tests/test_gpu_attention.py): four times
the worst absolute error of an fp32 torch evaluation of that output against
float64; u16 * |ref| for the 16-bit outputs y and dx; and the roundings the
kernels make by design, from the float64 quantities. h is rounded before fc2
and dW2: y gets u16 * (|h| |w2|^T), dw2 gets u16 * (|dy|^T |h|). dz is
rounded, and for GELU its factor gelu'(z) is taken at the stored 16-bit z,
so e = u16 * (|dz| + |z gelu''(z)| |dh|) with gelu''(z) = phi(z) (2 - z^2);
dx gets e |w1|, dw1 gets e^T |x|, db1 gets sum_m e. db2 has the base term
only. Every case runs twice: the same bits.

The chunk rule (two blocks per CU over the output tiles, whole 64-row steps)
splits M = 2056 at 256 x 1024 into 17 chunks of 128 rows, the last of 8.

Worst |kernel - ref| / bound over the cases, measured on an MI355X
(profiles/r19_mlp.md has the table): y 0.79, dx 0.55, dw1 0.76, db1 0.76,
dw2 0.91, db2 0.50.
"""

import math

import pytest
import torch

import mi355x.ops as ops
from _bn_pool_ref import u16

pytestmark = pytest.mark.gpu

BF, HF = torch.bfloat16, torch.float16

# (M, D, F, act, dtype)
CASES = {
    "one-row": (1, 64, 64, "gelu", BF),
    "one-tile": (128, 64, 128, "gelu", BF),
    "tiny-kn": (130, 8, 8, "gelu", BF),
    "tails": (200, 72, 136, "gelu", BF),
    "s-relu": (520, 192, 768, "relu", BF),
    "model-split": (2056, 256, 1024, "gelu", BF),
    "tails-fp16": (200, 72, 136, "gelu", HF),
    "dy-t": (200, 72, 136, "relu", BF),      # non-contiguous dy
    "saturated": (128, 64, 128, "gelu", BF),  # z reaches about +-8
}
OUTS = ("y", "dx", "dw1", "db1", "dw2", "db2")


def _inputs(name):
    M, D, F, act, dtype = CASES[name]
    g = torch.Generator().manual_seed(sorted(CASES).index(name))
    r = lambda *s: torch.randn(*s, generator=g)
    x = r(M, D) * (2.0 if name == "saturated" else 1.0)  # z ~ N(0, 4)
    w1, b1 = r(F, D) / math.sqrt(D), r(F) * 0.5
    w2, b2 = r(D, F) / math.sqrt(F), r(D) * 0.5
    dy = r(D, M).t() if name == "dy-t" else r(M, D)
    assert dy.is_contiguous() == (name != "dy-t")
    return [t.to(dtype).cuda() for t in (x, w1, b1, w2, b2, dy)]


def _kernel(act, x, w1, b1, w2, b2, dy):
    leaves = [x.clone().requires_grad_()] + [
        t.float().requires_grad_() for t in (w1, b1, w2, b2)]
    y = ops.mlp(*leaves, act=act)
    return [y.detach(), *torch.autograd.grad(y, leaves, dy)]


def _torch_eval(work, act, x, w1, b1, w2, b2, dy):
    """The six outputs in dtype `work`, and the design terms of the bound
    (without u16) in the order of OUTS."""
    leaves = [t.to(work).requires_grad_() for t in (x, w1, b1, w2, b2)]
    x, w1, b1, w2, b2 = leaves
    dy = dy.to(work)
    z = x @ w1.t() + b1
    cdf = 0.5 * (1 + torch.erf(z / math.sqrt(2)))
    h = z * cdf if act == "gelu" else torch.relu(z)
    y = h @ w2.t() + b2
    grads = torch.autograd.grad(y, leaves, dy)
    with torch.no_grad():
        dh = dy @ w2
        if act == "gelu":
            pdf = torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)
            dz = dh * (cdf + z * pdf)
            e = dz.abs() + (z * pdf * (2 - z * z)).abs() * dh.abs()
        else:
            e = (dh * (z > 0)).abs()
        terms = [h.abs() @ w2.abs().t(), e @ w1.abs(), e.t() @ x.abs(),
                 e.sum(0), dy.abs().t() @ h.abs(), torch.zeros_like(b2)]
    return [y.detach(), *grads], terms


@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_backward_against_float64(name):
    act, dtype = CASES[name][3:]
    ins = _inputs(name)
    got = _kernel(act, *ins)
    ref, terms = _torch_eval(torch.float64, act, *ins)
    f32, _ = _torch_eval(torch.float32, act, *ins)
    u = u16(dtype)
    worst = {}
    for key, k, r, f, term in zip(OUTS, got, ref, f32, terms):
        assert k.shape == r.shape and not torch.isnan(k).any(), key
        assert k.dtype == (dtype if key in ("y", "dx") else torch.float32)
        bound = 4 * (f.double() - r).abs().max() + u * term
        if key in ("y", "dx"):
            bound = bound + u * r.abs()
        err = (k.double() - r).abs()
        worst[key] = float((err / bound.clamp_min(1e-300)).max())
    print(f"mlp {name:12s} " + " ".join(f"{k}={r:.3f}"
                                        for k, r in worst.items()))
    assert all(r <= 1.0 for r in worst.values()), worst
    for a, b in zip(got, _kernel(act, *ins)):  # fixed order: the same bits
        assert torch.equal(a, b)


def test_captured_forward_backward_replays():
    """Capture form of tests/test_gpu_attention.py; two replays against
    eager."""
    act = "gelu"
    x, w1, b1, w2, b2, dy = _inputs("tails")
    want = _kernel(act, x, w1, b1, w2, b2, dy)
    leaves = [x.clone().requires_grad_()] + [
        t.float().requires_grad_() for t in (w1, b1, w2, b2)]

    def step():
        for t in leaves:
            t.grad = None
        y = ops.mlp(*leaves, act=act)
        y.backward(dy)
        return y

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = step()
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip([y.detach()] + [t.grad for t in leaves], want):
            assert torch.equal(a, b)
