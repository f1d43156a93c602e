"""csrc/gn.hip through fn._GNFn against float64 on the same 16-bit inputs.

Pass line, per case and output tensor: four times the worst absolute error
of an fp32 torch evaluation (F.group_norm on the fp32 upcast, residual,
ReLU, autograd; nothing rounded to 16 bits) against the float64 reference,
since the kernels sum in another order; the 16-bit outputs add
u16(dtype) * |ref| for their one rounding. The backward mask of all three
evaluations is the kernel's own y > 0.

Worst |kernel - ref| / bound over all cases, measured on an MI355X, is
recorded per output in profiles/r14_groupnorm.md.
"""

import pytest
import torch
import torch.nn.functional as F

import mi355x.ops as ops
from mi355x.ops import functional as fn
from _bn_pool_ref import u16

pytestmark = pytest.mark.gpu

BF, HF = torch.bfloat16, torch.float16
EPS = 1e-5

# (N, H, W, C, G, dtype, path, chunk, residual, relu, shift)
FIRST = (3, 5, 7, 64, 32)
CASES = {
    # ragged 35 pixels; cpg 2, 8, 64: groups in a lane, across lanes, a slab
    "res-cpg2": (*FIRST, BF, 1, 0, True, True, 0.0),
    "res-cpg2-nores": (*FIRST, BF, 1, 0, False, True, 0.0),
    "res-cpg2-norelu": (*FIRST, BF, 1, 0, True, False, 0.0),
    "res-cpg2-plain": (*FIRST, BF, 1, 0, False, False, 0.0),
    "res-cpg2-fp16": (*FIRST, HF, 1, 0, True, True, 0.0),
    "res-cpg8": (3, 5, 7, 64, 8, BF, 1, 0, True, True, 0.0),
    "res-cpg64": (3, 5, 7, 64, 1, BF, 1, 0, True, True, 0.0),
    "res-c8": (3, 5, 7, 8, 8, BF, 1, 0, True, True, 0.0),  # C < 64, cpg 1
    "res-c96": (3, 5, 7, 96, 12, BF, 1, 0, True, True, 0.0),  # 32-wide slabs
    # two slabs, four tiles a block, ten tiles: the last block is half empty
    "res-tiles": (5, 4, 4, 128, 4, BF, 1, 0, True, True, 0.0),
    # the forward's larger teams (256 and 1024 threads, 4 and 8 vectors a
    # lane), ragged; auto: their backward is the streamed one
    "res-t256-4": (2, 10, 10, 64, 32, BF, 0, 0, True, True, 0.0),
    "res-t256-8": (2, 15, 15, 64, 32, BF, 0, 0, True, True, 0.0),
    "res-t1024-4": (1, 20, 19, 64, 32, BF, 0, 0, True, True, 0.0),
    "res-t1024-8": (1, 24, 23, 64, 32, BF, 0, 0, True, True, 0.0),
    # three ragged chunks to combine
    "str-chunks": (*FIRST, BF, 2, 16, True, True, 0.0),
    "str-chunks-fp16": (*FIRST, HF, 2, 16, True, True, 0.0),
    "str-cpg128": (3, 5, 7, 128, 1, BF, 0, 0, True, True, 0.0),  # by rule
    "str-big": (2, 48, 48, 64, 32, BF, 0, 0, True, True, 0.0),   # by rule
    # mean >> std: the variance must be centred
    "res-shift": (*FIRST, BF, 1, 0, True, True, 64.0),
    "str-shift": (*FIRST, BF, 2, 16, True, True, 64.0),
}
NONCONTIG_DY = "res-cpg8"


def _inputs(name):
    N, H, W, C, G, dtype, path, chunk, has_res, relu, shift = CASES[name]
    g = torch.Generator().manual_seed(sorted(CASES).index(name))
    x = (shift + torch.randn(N, H, W, C, generator=g)).to(dtype).cuda()
    res = torch.randn(N, H, W, C, generator=g).to(dtype).cuda()
    gamma = 0.5 + torch.rand(C, generator=g)
    gamma[1], gamma[C - 2] = -0.7, -1.2
    beta = 0.3 * torch.randn(C, generator=g)
    if name == NONCONTIG_DY:
        dy = torch.randn(N, W, H, C, generator=g).to(dtype).cuda()
        dy = dy.transpose(1, 2)
        assert not dy.is_contiguous()
    else:
        dy = torch.randn(N, H, W, C, generator=g).to(dtype).cuda()
    return x, gamma.cuda(), beta.cuda(), res if has_res else None, dy


def _kernel(name, x, gamma, beta, res, dy):
    _, _, _, _, G, _, path, chunk, _, relu, _ = CASES[name]
    leaves = [t.clone().requires_grad_()
              for t in (x, gamma, beta) + ((res,) if res is not None else ())]
    y = fn._GNFn.apply(leaves[0], leaves[1], leaves[2],
                       leaves[3] if res is not None else None, G,
                       int(relu), EPS, True, path, chunk)
    grads = torch.autograd.grad(y, leaves, dy)
    out = dict(y=y.detach(), dx=grads[0], dgamma=grads[1], dbeta=grads[2])
    if res is not None:
        out["dres"] = grads[3]
    return out


def _torch_eval(work, name, x, gamma, beta, res, dy, keep):
    """y and the gradients in dtype `work`; the ReLU backward is `keep`."""
    G, relu = CASES[name][4], CASES[name][9]
    xd, gd, bd = (t.to(work).requires_grad_() for t in (x, gamma, beta))
    z = F.group_norm(xd.permute(0, 3, 1, 2), G, gd, bd, EPS)
    z = z.permute(0, 2, 3, 1)
    if res is not None:
        z = z + res.to(work)
    d = dy.to(work) * keep.to(work)
    dx, dgamma, dbeta = torch.autograd.grad(z, (xd, gd, bd), d)
    return dict(y=F.relu(z.detach()) if relu else z.detach(), dx=dx,
                dgamma=dgamma, dbeta=dbeta, dres=d)


@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_backward_against_float64(name):
    dtype, relu = CASES[name][5], CASES[name][9]
    inp = _inputs(name)
    got = _kernel(name, *inp)
    assert got["y"].dtype == dtype and got["dx"].dtype == dtype
    assert got["dgamma"].dtype == torch.float32
    keep = got["y"] > 0 if relu else torch.ones_like(got["y"],
                                                     dtype=torch.bool)
    if relu:  # both kinds of element were compared
        assert bool(keep.any()) and bool((~keep).any())
    ref = _torch_eval(torch.float64, name, *inp, keep)
    f32 = _torch_eval(torch.float32, name, *inp, keep)
    worst = {}
    for k, v in got.items():
        bound = 4 * (f32[k].double() - ref[k]).abs().max()
        if v.dtype == dtype:
            bound = bound + u16(dtype) * ref[k].abs()
        err = (v.double() - ref[k]).abs()
        worst[k] = float((err / bound.clamp_min(1e-300)).max())
    print(f"gn {name:16s} " + " ".join(f"{k}={r:.3f}"
                                       for k, r in worst.items()))
    assert all(r <= 1.0 for r in worst.values()), worst
    if "dres" in got:  # the masked dy itself
        want = torch.where(keep, inp[4], torch.zeros_like(inp[4]))
        assert torch.equal(got["dres"], want)
    again = _kernel(name, *inp)  # fixed-order reductions: the same bits
    assert all(torch.equal(got[k], again[k]) for k in got)


def test_nan_stays_in_its_group():
    name = "res-cpg8"
    x, gamma, beta, res, _ = _inputs(name)
    x[1, 2, 3, 17] = float("nan")  # sample 1, group 2 (channels 16..23)
    for path, chunk in ((1, 0), (2, 16)):
        with torch.no_grad():
            y = fn._GNFn.apply(x, gamma, beta, res, 8, 1, EPS, False, path,
                               chunk)
        bad = torch.zeros_like(y, dtype=torch.bool)
        bad[1, :, :, 16:24] = True
        assert torch.equal(torch.isnan(y), bad)


def test_captured_forward_backward_replays():
    """Capture form of tests/test_gpu_mix.py; two replays against eager."""
    name = "res-cpg2"
    x, gamma, beta, res, dy = _inputs(name)
    want = _kernel(name, x, gamma, beta, res, dy)
    static = [t.clone().requires_grad_() for t in (x, gamma, beta, res)]

    def step():
        for t in static:
            t.grad = None
        y = ops.group_norm(static[0], 32, static[1], static[2], static[3],
                           "relu", EPS)
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
        got = dict(y=y.detach(), dx=static[0].grad, dgamma=static[1].grad,
                   dbeta=static[2].grad, dres=static[3].grad)
        assert all(torch.equal(got[k], want[k]) for k in want)


def test_domain_and_path_errors_on_the_gpu():
    x = torch.zeros(2, 4, 4, 64, dtype=BF, device="cuda")
    w = torch.ones(64, device="cuda")
    with pytest.raises(ValueError, match="num_groups=5"):
        fn.group_norm(x, 5, w, w)
    with pytest.raises(ValueError, match=r"per group=\d+ .*power of two"):
        fn.group_norm(torch.zeros(2, 4, 4, 96, dtype=BF, device="cuda"), 8,
                      torch.ones(96, device="cuda"),
                      torch.ones(96, device="cuda"))
    with pytest.raises(ValueError, match="channels=12"):
        fn.group_norm(torch.zeros(2, 4, 4, 12, dtype=BF, device="cuda"), 3,
                      torch.ones(12, device="cuda"),
                      torch.ones(12, device="cuda"))
    # the resident path refuses what the rule sends to the streamed one
    for name in ("str-cpg128", "str-big"):
        inp = _inputs(name)
        with pytest.raises(RuntimeError, match="resident path"):
            fn._GNFn.apply(inp[0], inp[1], inp[2], inp[3], CASES[name][4], 1,
                           EPS, True, 1, 0)
