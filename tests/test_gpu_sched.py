"""The schedule / EMA variants of the update kernels and the clock kernel on
hardware: the scripted run (schedule, EMA, an overflowing step, a clipped
step) against the fp64 loop and the CPU twin's clock, a captured step
replayed over changing gradients against the same steps run eagerly, the
pointer-lr variant against the float-lr kernel, and EMA.swapped() against a
second model that loads the averaged weights.

Observed on an MI355X (more in profiles/r11_sched_ema.md), seven steps
against fp64, bound rtol 1e-5 / atol 1e-6: max |w - fp64| 5.9e-07, |m - fp64|
6.0e-07, |e - fp64| 5.4e-07 (SGD); 5.0e-07, 4.9e-07, 5.5e-07 (LARS). Every
other comparison here is bit for bit.
"""

import pytest
import torch

from _sched_common import (DECAY, INF_STEP, STEPS, build, inputs, reference,
                           run, snapshot)
from mi355x import amp, optim
from mi355x.models import Net
from mi355x.ops import cross_entropy
from mi355x.ops import functional as fn
from mi355x.parallel.flat import FlatState

pytestmark = pytest.mark.gpu

KINDS = ["sgd", "lars"]
NEVER_CLIPS = 1e30


@pytest.mark.parametrize("kind", KINDS)
def test_run_matches_fp64_and_the_cpu_twins_clock(kind):
    flat, opt, lrs, snaps, gbufs = run(kind, "cuda", clip_last=True)
    _, _, lrs_c, snaps_c, _ = run(kind, "cpu", clip_last=True)
    ref = reference(kind, True)
    assert len(snaps) == STEPS + 1
    assert lrs == lrs_c
    for k, (w, m, e, ick) in enumerate(snaps):
        rw, rm, re_, rt = ref[k]
        print(f"{kind} step {k + 1}: max |w - fp64| "
              f"{(w.double() - rw).abs().max():.3e}, |m - fp64| "
              f"{(m.double() - rm).abs().max():.3e}, |e - fp64| "
              f"{(e.double() - re_).abs().max():.3e}")
        torch.testing.assert_close(w.double(), rw, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(m.double(), rm, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(e.double(), re_, rtol=1e-5, atol=1e-6)
        # step count, lr and EMA weight: the twin's to the bit
        assert int(ick[fn.CK_STEP]) == rt
        assert torch.equal(ick, snaps_c[k][3])
    # the overflowing step wrote nothing, the one after it did
    for a, b in zip(snaps[INF_STEP - 1], snaps[INF_STEP]):
        assert torch.equal(a, b)
    for a, b in zip(snaps[INF_STEP], snaps[INF_STEP + 1]):
        assert not torch.equal(a, b)
    assert opt.skipped_steps == 1 and opt.clock_step == STEPS
    assert float(opt.last_grad_norm) > 10.0          # the last step clipped
    assert flat.sentinels_intact()
    _, _, grads = inputs()
    for k, g in enumerate(gbufs):                    # the gradient is read only
        assert torch.equal(g, grads[k])


def _five_steps(kind, captured):
    """Five steps through a DeviceGradScaler (the third overflows, the scale
    grows and backs off on the way), eagerly or as replays of one captured
    step. -> snapshots and scaler states after each."""
    w0, m0, grads = inputs()
    flat, opt = build(kind, "cuda")
    scaler = amp.DeviceGradScaler(init_scale=16.0, growth_interval=2,
                                  device="cuda")
    # side-stream warm-up (first-use allocations), then back to the start
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            flat.flat_grad.copy_(grads[STEPS])
            opt.step(scaler=scaler)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    flat.flat_param.copy_(w0)
    flat.flat_momentum.copy_(m0)
    opt.ema.flat_ema.copy_(w0)
    fn.clock_set(opt.clock, 0, opt._table, DECAY, True)
    scaler.state.copy_(fn.new_guard_state("cuda", scale=16.0))
    graph = None
    if captured:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            opt.step(scaler=scaler)
    out = []
    for k in range(5):
        flat.flat_grad.copy_(grads[k])     # the only host work per step
        if captured:
            graph.replay()
        else:
            opt.step(scaler=scaler)
        out.append(snapshot(flat, opt) + (scaler.state.cpu().clone(),))
    assert flat.sentinels_intact()
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_captured_step_follows_schedule_and_skips_by_itself(kind):
    eager = _five_steps(kind, captured=False)
    replayed = _five_steps(kind, captured=True)
    for k, (a, b) in enumerate(zip(eager, replayed)):
        for x, y in zip(a, b):
            assert torch.equal(x, y), k
    steps = [int(s[3][fn.CK_STEP]) for s in replayed]
    assert steps == [1, 2, 2, 3, 4]
    lrs = [float(s[3].view(torch.float32)[fn.CK_LR]) for s in replayed]
    assert len(set(lrs)) == 4 and lrs[1] == lrs[2]   # nobody wrote the lr
    for x, y in zip(replayed[INF_STEP - 1][:4], replayed[INF_STEP][:4]):
        assert torch.equal(x, y)
    scales = [float(s[4][fn.GS_SCALE]) for s in replayed]
    assert scales == [16.0, 32.0, 16.0, 16.0, 32.0]


@pytest.mark.parametrize("kind", KINDS)
def test_constant_table_is_the_guarded_float_lr_step(kind):
    _, _, grads = inputs()
    arms = {
        "table": build(kind, "cuda", lr=optim.LRSchedule([0.1] * 3),
                       ema=False),
        "float": build(kind, "cuda", lr=0.1, ema=False),
        "table_ema": build(kind, "cuda", lr=optim.LRSchedule([0.1] * 3)),
        "float_ema": build(kind, "cuda", lr=0.1),
    }
    for flat, opt in arms.values():
        opt.max_grad_norm = NEVER_CLIPS      # the guarded path for every arm
        for g in grads[:2] + grads[3:5]:     # four clean steps: past the table
            flat.flat_grad.copy_(g)
            opt.step()
        assert flat.sentinels_intact()
    assert arms["float"][1].clock is None
    assert arms["table"][1].clock_step == 4
    for a, b in (("table", "float"), ("table_ema", "float_ema"),
                 ("table_ema", "table")):
        fa, fb = arms[a][0], arms[b][0]
        assert torch.equal(fa.flat_param, fb.flat_param), (a, b)
        assert torch.equal(fa.flat_momentum, fb.flat_momentum), (a, b)
    assert torch.equal(arms["table_ema"][1].ema.flat_ema,
                       arms["float_ema"][1].ema.flat_ema)
    w0, _, _ = inputs()
    assert not torch.equal(arms["table"][0].flat_param.cpu(), w0)
    assert not torch.equal(arms["table_ema"][1].ema.flat_ema,
                           arms["table_ema"][0].flat_param)


def test_swapped_forward_uses_the_ema_weights():
    dev = torch.device("cuda")
    torch.manual_seed(0)
    net = Net().to(dev)
    flat = FlatState(net)
    ema = optim.EMA(0.9)
    opt = optim.SGD(flat, lr=0.5, momentum=0.9, ema=ema)
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(16, 3, 32, 32, generator=gen).to(dev)
    y = torch.randint(0, 10, (16,), generator=gen).to(dev)
    for _ in range(2):
        opt.zero_grad()
        cross_entropy(net(x), y).backward()
        opt.step()
    assert not torch.equal(ema.flat_ema, flat.flat_param)
    net.eval()
    with torch.no_grad():
        outside = net(x)          # fills the 16-bit weight cache
        with ema.swapped():
            inside = net(x)
            sd = {k: v.clone() for k, v in net.state_dict().items()}
        again = net(x)
        other = Net().to(dev)
        other.load_state_dict(sd)
        other.eval()
        expect = other(x)
    assert torch.equal(inside, expect)      # stale cached weights would differ
    assert not torch.equal(inside, outside)
    assert torch.equal(again, outside)
