"""csrc/se.hip through fn._SEFn against float64 on the same 16-bit inputs.

Pass line (that of tests/test_gpu_groupnorm.py), per case and output tensor:
four times the worst absolute error of an fp32 torch evaluation (the op's
formulas on the fp32 upcast, autograd; nothing rounded to 16 bits) against
the float64 reference, since the kernels sum in another order; the 16-bit
outputs add u16(dtype) * |ref| for their one rounding. The backward mask of
all three evaluations is the kernel's own y > 0.

Worst |kernel - ref| / bound over all cases, measured on an MI355X, is
recorded per output in profiles/r15_se.md.
"""

import pytest
import torch

import mi355x.ops as ops
from mi355x.ops import functional as fn
from _bn_pool_ref import u16

pytestmark = pytest.mark.gpu

BF, HF = torch.bfloat16, torch.float16

# (N, H, W, C, Cr, dtype, path, chunk, residual, relu)
BASE = (3, 5, 7, 64, 4)
CASES = {
    # 35 ragged pixels on a team of 64
    "res": (*BASE, BF, 1, 0, True, True),
    "res-nores": (*BASE, BF, 1, 0, False, True),
    "res-norelu": (*BASE, BF, 1, 0, True, False),
    "res-plain": (*BASE, BF, 1, 0, False, False),
    "res-fp16": (*BASE, HF, 1, 0, True, True),
    "res-dy-t": (*BASE, BF, 1, 0, True, True),  # non-contiguous dy
    "res-c8": (3, 5, 7, 8, 1, BF, 1, 0, True, True),
    "res-c96": (3, 5, 7, 96, 6, BF, 1, 0, True, True),  # 12 columns, 5 rows
    "res-c512": (2, 2, 2, 512, 32, BF, 1, 0, True, True),
    "res-c2048": (1, 1, 1, 2048, 128, BF, 1, 0, True, True),  # HW = 1
    # four teams a block, five samples: the last block is part empty
    "res-pack": (5, 4, 4, 128, 8, BF, 1, 0, True, True),
    # the larger teams and vector counts, ragged, as the rule picks them
    "auto-10x10": (2, 10, 10, 64, 4, BF, 0, 0, True, True),
    "auto-15x15": (2, 15, 15, 64, 4, BF, 0, 0, True, True),
    "auto-20x19": (1, 20, 19, 64, 4, BF, 0, 0, True, True),
    "auto-24x23": (1, 24, 23, 64, 4, BF, 0, 0, True, True),
    # three ragged chunks to add
    "str-chunks": (*BASE, BF, 2, 16, True, True),
    "str-chunks-fp16": (*BASE, HF, 2, 16, True, True),
    "str-big": (2, 48, 48, 64, 4, BF, 0, 0, True, True),  # by rule
    # logits of +30, -30, +120, -120 on channels 0..3
    "res-saturated": (*BASE, BF, 1, 0, True, True),
}
NAMES = ("y", "dx", "dw1", "db1", "dw2", "db2", "dres")


def _inputs(name):
    N, H, W, C, Cr, dtype, _, _, has_res, _ = CASES[name]
    g = torch.Generator().manual_seed(sorted(CASES).index(name))
    x = torch.randn(N, H, W, C, generator=g).to(dtype).cuda()
    res = torch.randn(N, H, W, C, generator=g).to(dtype).cuda()
    w1 = torch.randn(Cr, C, generator=g) / C ** 0.5
    b1 = 0.3 * torch.randn(Cr, generator=g)
    w2 = torch.randn(C, Cr, generator=g) / Cr ** 0.5
    b2 = 0.3 * torch.randn(C, generator=g)
    if name == "res-saturated":
        b2[:4] = torch.tensor([30.0, -30.0, 120.0, -120.0])
    if name == "res-dy-t":
        dy = torch.randn(N, W, H, C, generator=g).to(dtype).cuda()
        dy = dy.transpose(1, 2)
        assert not dy.is_contiguous()
    else:
        dy = torch.randn(N, H, W, C, generator=g).to(dtype).cuda()
    return (x, w1.cuda(), b1.cuda(), w2.cuda(), b2.cuda(),
            res if has_res else None, dy)


def _kernel(name, x, w1, b1, w2, b2, res, dy):
    path, chunk, relu = CASES[name][6], CASES[name][7], CASES[name][9]
    leaves = [t.clone().requires_grad_()
              for t in (x, w1, b1, w2, b2) + ((res,) if res is not None
                                              else ())]
    y = fn._SEFn.apply(*leaves[:5], leaves[5] if res is not None else None,
                       int(relu), True, path, chunk)
    grads = torch.autograd.grad(y, leaves, dy)
    return dict(zip(NAMES, (y.detach(),) + grads))


def _torch_eval(work, name, x, w1, b1, w2, b2, res, dy, keep):
    """y and the gradients in dtype `work`; the ReLU backward is `keep`."""
    relu = CASES[name][9]
    xd, w1d, b1d, w2d, b2d = (t.to(work).requires_grad_()
                              for t in (x, w1, b1, w2, b2))
    s = xd.mean(dim=(1, 2))
    z = torch.relu(s @ w1d.t() + b1d)
    g = torch.sigmoid(z @ w2d.t() + b2d)
    v = xd * g[:, None, None, :]
    if res is not None:
        v = v + res.to(work)
    d = dy.to(work) * keep.to(work)
    grads = torch.autograd.grad(v, (xd, w1d, b1d, w2d, b2d), d)
    y = torch.relu(v.detach()) if relu else v.detach()
    return dict(zip(NAMES, (y,) + grads + (d,)))


@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_backward_against_float64(name):
    dtype, relu = CASES[name][5], CASES[name][9]
    inp = _inputs(name)
    got = _kernel(name, *inp)
    assert got["y"].dtype == dtype and got["dx"].dtype == dtype
    assert all(got[k].dtype == torch.float32 and got[k].shape == t.shape
               for k, t in zip(NAMES[2:6], inp[1:5]))
    assert not any(torch.isnan(v).any() for v in got.values())
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
    print(f"se {name:16s} " + " ".join(f"{k}={r:.3f}"
                                       for k, r in worst.items()))
    assert all(r <= 1.0 for r in worst.values()), worst
    if "dres" in got:  # the masked dy itself
        want = torch.where(keep, inp[6], torch.zeros_like(inp[6]))
        assert torch.equal(got["dres"], want)
    if name == "res-saturated":  # a gate of exactly 0 leaves the residual
        assert torch.equal(got["y"][..., 3], torch.relu(inp[5][..., 3]))
    again = _kernel(name, *inp)  # fixed-order reductions: the same bits
    assert all(torch.equal(got[k], again[k]) for k in got)


def test_nan_stays_in_its_sample():
    inp = _inputs("res")
    x = inp[0].clone()
    x[1, 2, 3, 17] = float("nan")
    for path, chunk in ((1, 0), (2, 16)):
        with torch.no_grad():
            y = fn._SEFn.apply(x, *inp[1:6], 1, False, path, chunk)
        bad = torch.zeros_like(y, dtype=torch.bool)
        bad[1] = True
        assert torch.equal(torch.isnan(y), bad)


def test_captured_forward_backward_replays():
    """Capture form of tests/test_gpu_mix.py; two replays against eager."""
    inp = _inputs("res")
    dy = inp[6]
    want = _kernel("res", *inp)
    static = [t.clone().requires_grad_() for t in inp[:6]]

    def step():
        for t in static:
            t.grad = None
        y = ops.squeeze_excite(*static, "relu")
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
        got = dict(zip(NAMES, [y.detach()] + [t.grad for t in static]))
        assert all(torch.equal(got[k], want[k]) for k in want)


def test_domain_and_path_errors_on_the_gpu():
    x, w1, b1, w2, b2, _, _ = _inputs("res")
    with pytest.raises(ValueError, match="channels=12"):
        fn.squeeze_excite(x[..., :12], w1, b1, w2, b2)
    with pytest.raises(ValueError, match=r"b1 .*\(5,\)"):
        fn.squeeze_excite(x, w1, torch.zeros(5, device="cuda"), w2, b2)
    with pytest.raises(ValueError, match="residual .*float16"):
        fn.squeeze_excite(x, w1, b1, w2, b2, x.to(HF))
    # the resident path refuses what the rule sends to the streamed one
    inp = _inputs("str-big")
    with pytest.raises(RuntimeError, match="resident path"):
        fn._SEFn.apply(*inp[:6], 1, True, 1, 0)
