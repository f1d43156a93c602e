"""The adam.hip kernels on hardware through optim.AdamW / optim.LAMB, on the
tensor table of _lars_common (every head/body/tail split, excluded tensors,
zero weights, zero gradient): three steps against float64, a non-finite
gradient in a scalar tail, untouched neighbours of padded buffers, and a
captured step against the eager one.

Observed on an MI355X (per case in profiles/r16_adam.md): w, m and v at
most 0.041 of their line (rtol 4e-6, atol 4e-7), trust ratios at most
2.0e-07 relative (line 1e-5).
"""

import pytest
import torch

from _adam_common import (CASES, HP, OFF, compare, make, reference, run,
                          snapshot, start)
from _lars_common import EXCLUDE, ZERO_G, ZERO_W, synthetic
from mi355x import ops, optim
from mi355x.ops import functional as fn

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", list(CASES))
def test_three_steps_match_fp64(case):
    kind, max_norm, wd, exclude = CASES[case]
    w0, grads = start()
    ref = reference(kind, w0, grads, max_norm, wd, exclude)
    first = run(make(kind, w0, "cuda", max_norm, wd, exclude), grads)
    for k, got in enumerate(first):
        compare(got, ref[k], f"{case} step {k + 1}")
        if kind == "lamb":
            one = [s for s, ex in enumerate(EXCLUDE) if ex]
            one += [ZERO_W] if k == 0 else []
            one += [ZERO_G] if wd == 0.0 else []
            assert [s for s, t in enumerate(got[3]) if t == 1.0] == sorted(one)
    again = run(make(kind, w0, "cuda", max_norm, wd, exclude), grads)
    for a, b in zip(first, again):
        for x, y in zip(a, b):
            assert x is None or torch.equal(x, y)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
@pytest.mark.parametrize("kind", ["adamw", "lamb"])
def test_non_finite_gradient_writes_nothing_and_stops_the_clock(kind, bad):
    w0, good = start()
    poisoned = good[1].clone()
    # the end of tensor 7, 8191 elements from 2 modulo 4: its last tile has
    # a head of 2, 1023 vectors and a scalar tail of 1
    assert OFF[7] % 4 == 2
    poisoned[OFF[8] - 1] = bad
    opt = make(kind, w0, "cuda", 1.0, 1e-2, EXCLUDE, ema=optim.EMA(0.9))
    run(opt, good[:1])
    before = snapshot(opt) + [opt.ema.flat_ema.cpu().clone()]
    run(opt, [poisoned])
    for x, y in zip(before, snapshot(opt) + [opt.ema.flat_ema.cpu()]):
        assert x is None or torch.equal(x, y)
    assert opt.skipped_steps == 1 and opt.clock_step == 1
    end = run(opt, good[1:])[-1]
    assert opt.skipped_steps == 1 and opt.clock_step == 3
    compare(end, reference(kind, w0, good, 1.0, 1e-2, EXCLUDE)[-1],
            f"{kind} around a skipped step")


@pytest.mark.parametrize("kind", ["adamw", "lamb"])
def test_neighbours_stay_intact(kind):
    """test_gpu_lars' check for the passes LARS does not have: w, g, m, v
    and the EMA buffer between 16 floats of sentinel each; one step changes
    all but g and no sentinel."""
    w, m, (g,) = synthetic(steps=1)
    n, pad = OFF[-1], 16
    src = {"w": w, "g": g, "m": m, "v": m.square(), "e": w + 1.0}
    bufs = {}
    for name, t in src.items():
        b = torch.full((n + 2 * pad,), 12345.0, device="cuda")
        b[pad:pad + n] = t.cuda()
        bufs[name] = b
    view = {name: b[pad:pad + n] for name, b in bufs.items()}
    plan = ops.lars_plan(OFF, EXCLUDE, "cuda")
    st = fn.new_guard_state("cuda")
    clock = fn.new_clock("cuda", torch.zeros(1, device="cuda"), 0.9)
    ops.grad_stats(view["g"], out=st[fn.GS_NONFINITE:fn.GS_RAW_NORM + 1])
    step = ops.adam_step if kind == "adamw" else ops.lamb_step
    step(view["w"], view["g"], view["m"], view["v"], plan, st, clock,
         HP["lr"], HP["betas"], HP["eps"], 1e-2, HP["grad_scale"],
         ema=view["e"])
    assert int(st.view(torch.int32)[fn.GS_NONFINITE]) == 0
    guard = torch.full((pad,), 12345.0)
    for name, b in bufs.items():
        assert torch.equal(b[:pad].cpu(), guard), name
        assert torch.equal(b[pad + n:].cpu(), guard), name
        assert torch.equal(view[name].cpu(), src[name]) == (name == "g"), name


def _scheduled(kind, w0):
    return make(kind, w0, "cuda", 1.0, 1e-2, EXCLUDE, ema=optim.EMA(0.9),
                lr=optim.LRSchedule([1e-2, 2e-2, 5e-3, 1e-3]))


def _everything(opt):
    return snapshot(opt)[:3] + [opt.ema.flat_ema.cpu(),
                                opt.clock.view(torch.int32).cpu()]


@pytest.mark.parametrize("kind", ["adamw", "lamb"])
def test_captured_step_replays_like_the_eager_one(kind):
    w0, grads = start()
    eager = _scheduled(kind, w0)
    run(eager, grads)

    opt = _scheduled(kind, w0)
    sd0 = {k: v.clone() if isinstance(v, torch.Tensor) else v
           for k, v in opt.state_dict().items()}
    opt.flat.flat_grad.copy_(grads[0])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            opt.step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    # back to the start, in place: the graph keeps its pointers
    opt.flat.flat_param.copy_(w0)
    opt.load_state_dict(sd0)
    assert opt.clock_step == 0
    for g in grads:
        opt.flat.flat_grad.copy_(g)
        graph.replay()
    assert opt.clock_step == 3 and float(opt.lr) == pytest.approx(1e-3)
    assert int(opt.clock.view(torch.int32)[fn.CK_STEP]) == 3
    for x, y in zip(_everything(opt), _everything(eager)):
        assert torch.equal(x, y)
