"""The learning-rate schedule, the step clock and the weight EMA on the CPU
(the plain-torch twins of the kernels): the schedule builders against an
independent float64 evaluation, the clock through a run with a skipped
step, the EMA against an explicit fp64 loop, checkpoints, EMA.swapped(),
and both training scripts with MI355X_SCHED / MI355X_WARMUP_EPOCHS /
MI355X_EMA."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from _sched_common import (DECAY, INF_STEP, N, OFF, SIZES, PaddedFlat, build,
                           cosine_f64, f32, inputs, omd_f64, poly_f64,
                           reference, run, schedule, snapshot)
from mi355x import optim
from mi355x.models import Net
from mi355x.ops import functional as fn
from mi355x.parallel.flat import FlatState

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["sgd", "lars"]


def _ulps_apart(got_f32, ref_f64):
    """Distance in float32 steps between a float32 array and a float64
    array rounded to float32 (all values >= 0: the bit patterns order)."""
    a = np.asarray(got_f32, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(ref_f64, dtype=np.float64).astype(np.float32).view(
        np.int32).astype(np.int64)
    return np.abs(a - b)


def test_layout():
    assert N == 12359 and N % 4 == 3
    assert [o % 4 for o in OFF[:-1]] == [0, 1, 0, 1, 3]
    assert SIZES[1] > 4096 and SIZES[3] > 4096 and SIZES[2] == 1


BUILDER_CASES = [
    dict(base=0.1, W=5, T=40, end=0.0, start=0.0),
    dict(base=3.2, W=7, T=100, end=0.001, start=0.01),
    dict(base=0.4, W=0, T=17, end=0.0, start=0.0),
    dict(base=0.05, W=1, T=3, end=0.002, start=0.0),
]


@pytest.mark.parametrize("c", BUILDER_CASES)
@pytest.mark.parametrize("shape", ["cosine", "poly2", "poly1"])
def test_builders_match_float64_formula(c, shape):
    args = (c["base"], c["W"], c["T"])
    kw = dict(end_lr=c["end"], warmup_start=c["start"])
    if shape == "cosine":
        s = optim.LRSchedule.warmup_cosine(*args, **kw)
        ref = [cosine_f64(t, c["base"], c["W"], c["T"], c["end"], c["start"])
               for t in range(c["T"])]
    else:
        power = 2.0 if shape == "poly2" else 1.0
        s = optim.LRSchedule.warmup_poly(*args, power=power, **kw)
        ref = [poly_f64(t, c["base"], c["W"], c["T"], c["end"], c["start"],
                        power) for t in range(c["T"])]
    v = s.values
    assert v.dtype == torch.float32 and v.shape == (c["T"],) == (len(s),)
    if c["W"] > 0:
        assert float(v[0]) == f32(c["start"])
    assert float(v[c["W"]]) == f32(c["base"])
    assert float(v[-1]) == f32(c["end"])
    # two double evaluations a few double-ulps apart can round to
    # neighbouring floats, never further
    assert int(_ulps_apart(v.numpy(), ref).max()) <= 1
    if c["W"] > 1:
        assert bool((v[1:c["W"] + 1] > v[:c["W"]]).all())     # warm-up rises
    assert bool((v[c["W"] + 1:] <= v[c["W"]:-1]).all())       # then decays


def test_constructor_round_trips_and_validates():
    vals = np.array([0.1, 0.30000001192092896, 1e-8, 0.0, 7.5],
                    dtype=np.float32)
    for given in (vals.tolist(), torch.from_numpy(vals.copy()), vals):
        s = optim.LRSchedule(given)
        assert s.values.dtype == torch.float32
        assert np.array_equal(s.values.numpy().view(np.int32),
                              vals.view(np.int32))
    assert float(optim.LRSchedule([0.1]).values[0]) == f32(0.1)  # one rounding
    with pytest.raises(ValueError):
        optim.LRSchedule([])
    with pytest.raises(ValueError):
        optim.LRSchedule([0.1, float("nan")])
    with pytest.raises(ValueError):
        optim.EMA(1.0)


def test_clock_advance_twin_follows_the_formula():
    table = optim.LRSchedule([0.5, 0.25, 0.125]).values
    for decay, warmup in ((0.5, True), (0.999, True), (0.9, False)):
        clock = fn.new_clock("cpu", table, decay, warmup)
        state = fn.new_guard_state("cpu")
        for t in range(0, 12):
            ick = clock.view(torch.int32)
            assert int(ick[fn.CK_STEP]) == t
            assert float(clock[fn.CK_LR]) == float(table[min(t, 2)])
            assert float(clock[fn.CK_EMA_OMD]) == f32(
                omd_f64(t, decay, warmup))
            state.view(torch.int32)[fn.GS_NONFINITE] = 3
            before = ick.clone()
            fn.clock_advance(clock, state, table, decay, warmup)
            assert torch.equal(clock.view(torch.int32), before)   # skipped
            state.view(torch.int32)[fn.GS_NONFINITE] = 0
            fn.clock_advance(clock, state if t % 2 else None, table, decay,
                             warmup)
    # the decay itself takes over from the warm-up: (1 + 8) / (10 + 8) = 0.5
    assert omd_f64(7, 0.5) > 0.5 and omd_f64(8, 0.5) == 0.5 == omd_f64(11, 0.5)


@pytest.mark.parametrize("kind", KINDS)
def test_clock_through_a_run_with_a_skipped_step(kind):
    table = schedule().values
    T = len(table)
    flat, opt, lrs, snaps, gbufs = run(kind, "cpu")
    applied = [0, 1, 2, 2, 3, 4]          # applied steps before each step
    assert lrs == [float(table[min(t, T - 1)]) for t in applied]
    assert lrs[INF_STEP] == lrs[INF_STEP + 1]         # the skip repeats its lr
    for k, (_, _, _, ick) in enumerate(snaps):
        t = applied[k] + (0 if k == INF_STEP else 1)
        assert int(ick[fn.CK_STEP]) == t
        ck = ick.view(torch.float32)
        assert float(ck[fn.CK_LR]) == float(table[min(t, T - 1)])
        assert float(ck[fn.CK_EMA_OMD]) == f32(omd_f64(t))
    assert opt.clock_step == 5 and opt.skipped_steps == 1
    assert isinstance(opt.lr, torch.Tensor) and opt.lr.dim() == 0
    assert opt.lr.data_ptr() == opt.clock[fn.CK_LR].data_ptr()
    # the skipped step: w, m, e and the clock bit-unchanged
    for a, b in zip(snaps[INF_STEP - 1], snaps[INF_STEP]):
        assert torch.equal(a, b)
    for a, b in zip(snaps[INF_STEP], snaps[INF_STEP + 1]):
        assert not torch.equal(a, b)
    assert flat.sentinels_intact()
    _, _, grads = inputs()
    for k, g in enumerate(gbufs):                     # the gradient is read only
        assert torch.equal(g, grads[k])


@pytest.mark.parametrize("kind", KINDS)
def test_ema_and_update_match_fp64_loop(kind):
    _, _, _, snaps, _ = run(kind, "cpu")
    ref = reference(kind)
    for k, (w, m, e, ick) in enumerate(snaps):
        rw, rm, re_, rt = ref[k]
        print(f"{kind} step {k + 1}: max |w - fp64| "
              f"{(w.double() - rw).abs().max():.3e}, |m - fp64| "
              f"{(m.double() - rm).abs().max():.3e}, |e - fp64| "
              f"{(e.double() - re_).abs().max():.3e}")
        torch.testing.assert_close(w.double(), rw, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(m.double(), rm, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(e.double(), re_, rtol=1e-5, atol=1e-6)
        assert int(ick[fn.CK_STEP]) == rt
    # warm-up: d_0 = 1/10, so the first applied step leaves 0.9 w_1 + 0.1 w_0
    w0, _, _ = inputs()
    w1, _, e1, _ = snaps[0]
    torch.testing.assert_close(e1.double(),
                               0.9 * w1.double() + 0.1 * w0.double(),
                               rtol=1e-5, atol=1e-6)
    assert not torch.equal(e1, w1)


@pytest.mark.parametrize("kind", KINDS)
def test_constant_table_without_ema_is_the_float_lr_optimizer(kind):
    _, _, grads = inputs()
    flat_s, opt_s = build(kind, "cpu", lr=optim.LRSchedule([0.1] * 3),
                          ema=False)
    flat_f, opt_f = build(kind, "cpu", lr=0.1, ema=False)
    assert opt_f.clock is None and opt_s.ema is None
    for g in grads[:2] + grads[3:5]:      # four clean steps: past the table
        for flat, opt in ((flat_s, opt_s), (flat_f, opt_f)):
            flat.flat_grad.copy_(g)
            opt.step()
    assert opt_s.clock_step == 4
    assert torch.equal(flat_s.flat_param, flat_f.flat_param)
    assert torch.equal(flat_s.flat_momentum, flat_f.flat_momentum)
    w0, _, _ = inputs()
    assert not torch.equal(flat_s.flat_param, w0)


def test_swapped_exchanges_restores_and_changes_the_output():
    torch.manual_seed(0)
    net = Net()
    flat = FlatState(net)
    ema = optim.EMA(0.9)
    opt = optim.SGD(flat, lr=0.5, momentum=0.9, ema=ema)
    assert torch.equal(ema.flat_ema, flat.flat_param)
    assert ema.flat_ema.data_ptr() != flat.flat_param.data_ptr()
    flat.flat_grad.copy_(torch.randn(flat.numel))
    opt.step()
    x = torch.randn(4, 3, 32, 32)
    net.eval()
    with torch.no_grad():
        outside = net(x)
    w, e = flat.flat_param.clone(), ema.flat_ema.clone()
    assert not torch.equal(w, e)
    ptr = flat.flat_param.data_ptr()
    epoch = fn._cache_epoch
    with ema.swapped() as inside_ema:
        assert inside_ema is ema and fn._cache_epoch == epoch + 1
        assert torch.equal(flat.flat_param, e)
        assert torch.equal(ema.flat_ema, w)
        assert flat.flat_param.data_ptr() == ptr      # contents, not pointers
        with torch.no_grad():
            inside = net(x)
    assert fn._cache_epoch == epoch + 2
    assert torch.equal(flat.flat_param, w) and torch.equal(ema.flat_ema, e)
    assert not torch.equal(inside, outside)
    with torch.no_grad():
        assert torch.equal(net(x), outside)
    with pytest.raises(RuntimeError):
        with optim.EMA(0.9).swapped():
            pass


@pytest.mark.parametrize("kind", KINDS)
def test_state_dict_round_trip_resumes_lr_and_ema(kind):
    _, _, grads = inputs()
    flat_a, opt_a = build(kind, "cpu")
    for g in grads[:4]:                   # three applied steps and the skip
        flat_a.flat_grad.copy_(g)
        opt_a.step()
    sd = opt_a.state_dict()
    assert sd["clock_step"] == 3 and isinstance(sd["clock_step"], int)
    assert isinstance(sd["lr"], float) and sd["lr"] == float(opt_a.lr)
    assert sd["ema_decay"] == DECAY and sd["ema_warmup"] is True
    assert torch.equal(sd["ema"], opt_a.ema.flat_ema)
    saved = {k: (v.clone() if isinstance(v, torch.Tensor) else v)
             for k, v in sd.items()}

    flat_b, opt_b = build(kind, "cpu", w=torch.zeros(N), m=torch.zeros(N))
    clock_ptr, ema_ptr = opt_b.clock.data_ptr(), opt_b.ema.flat_ema.data_ptr()
    flat_b.flat_param.copy_(flat_a.flat_param)        # the model's checkpoint
    opt_b.load_state_dict(saved)
    assert opt_b.clock.data_ptr() == clock_ptr        # restored in place
    assert opt_b.ema.flat_ema.data_ptr() == ema_ptr
    for a, b in zip(snapshot(flat_a, opt_a), snapshot(flat_b, opt_b)):
        assert torch.equal(a, b)
    for g in grads[4:6]:
        for flat, opt in ((flat_a, opt_a), (flat_b, opt_b)):
            flat.flat_grad.copy_(g)
            opt.step()
    assert opt_b.clock_step == 5
    for a, b in zip(snapshot(flat_a, opt_a), snapshot(flat_b, opt_b)):
        assert torch.equal(a, b)


def test_checkpoint_without_the_new_keys_still_loads():
    w, m, _ = inputs()
    old = {"momentum_buffer": m * 2, "lr": 0.25, "momentum": 0.8,
           "weight_decay": 5e-4}
    flat, opt = build("sgd", "cpu", lr=0.1, ema=False)        # as before
    opt.load_state_dict(old)
    assert opt.lr == 0.25 and opt.momentum == 0.8 and opt.clock_step == 0
    assert torch.equal(flat.flat_momentum, m * 2)
    assert set(old) | {"max_grad_norm", "clock_step"} == set(opt.state_dict())

    flat, opt = build("sgd", "cpu")                           # schedule + EMA
    flat.flat_grad.copy_(torch.ones(N))
    opt.step()
    flat.flat_param.copy_(w * 3)                              # the model loads
    opt.load_state_dict(old)
    assert opt.clock_step == 0
    assert float(opt.lr) == float(schedule().values[0])       # not the saved lr
    assert float(opt.clock[fn.CK_EMA_OMD]) == f32(omd_f64(0))
    assert torch.equal(opt.ema.flat_ema, w * 3)               # re-seeded
    assert torch.equal(flat.flat_momentum, m * 2)


def test_from_env_and_describe(monkeypatch):
    for k in ("MI355X_OPTIM", "MI355X_WD", "MI355X_SCHED",
              "MI355X_WARMUP_EPOCHS", "MI355X_EMA"):
        monkeypatch.delenv(k, raising=False)
    assert optim.schedule_from_env(0.3, 100, 2) == 0.3
    assert optim.ema_from_env() is None
    monkeypatch.setenv("MI355X_EMA", "0")
    assert optim.ema_from_env() is None
    monkeypatch.setenv("MI355X_EMA", "0.999")
    monkeypatch.setenv("MI355X_SCHED", "poly")
    monkeypatch.setenv("MI355X_WARMUP_EPOCHS", "0.5")
    s = optim.schedule_from_env(0.3, 100, 2)
    assert len(s) == 200 and float(s.values[50]) == f32(0.3)
    assert float(s.values[0]) == 0.0 and float(s.values[-1]) == 0.0
    ema = optim.ema_from_env()
    assert ema.decay == 0.999 and ema.warmup
    w, m, _ = inputs()
    opt = optim.from_env(PaddedFlat(w, m, "cpu"), lr=s, ema=ema)
    assert type(opt) is optim.SGD and opt.ema is ema and opt.schedule is s
    assert optim.describe(opt) == ("SGD lr=0 momentum=0.9 weight_decay=0 "
                                   "schedule=200 steps ema=0.999")
    monkeypatch.setenv("MI355X_SCHED", "step")
    with pytest.raises(ValueError, match="expected const, cosine or poly"):
        optim.schedule_from_env(0.3, 100, 2)


# ---------------------------------------------------------------------------
# the training scripts
# ---------------------------------------------------------------------------

KNOBS = {
    "MI355X_SYNTHETIC": "1",
    "MI355X_STEPS": "3",
    "MI355X_EPOCHS": "1",
    "MI355X_BATCH": "8",
    "MI355X_LR": "0.05",
}
SCHED = {
    "MI355X_SCHED": "cosine",
    "MI355X_WARMUP_EPOCHS": "0.5",
    "MI355X_EMA": "0.99",
}
SERIAL = [sys.executable, "cifar_example.py"]


def _ddp(port):
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
            "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
            "--master-port", str(port), "cifar_example_ddp.py"]


def _run(cmd, extra_env, timeout=600):
    env = dict(os.environ)
    for k in SCHED:
        env.pop(k, None)
    env.update(extra_env)
    return subprocess.run(cmd, cwd=REPO, env=env, capture_output=True,
                          text=True, timeout=timeout)


def _ema_lines(r):
    return [ln for ln in r.stdout.splitlines() if "EMA" in ln]


@pytest.mark.parametrize("script", ["serial", "ddp"])
def test_scripts_with_schedule_and_ema(tmp_path, script):
    ckpt = tmp_path / "net.pth"
    cmd = SERIAL if script == "serial" else _ddp(29743)
    r = _run(cmd, dict(KNOBS, **SCHED, MI355X_CKPT=str(ckpt)))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Finished Training (3 steps" in r.stdout
    assert len(_ema_lines(r)) == 1, r.stdout[-2000:]
    assert _ema_lines(r)[0].startswith("Accuracy of the EMA weights")
    # total_steps = epochs * len(train loader): 50000 / 8, per rank
    total = 6250 if script == "serial" else 3125
    assert ("optimizer: SGD lr=0 momentum=0.9 weight_decay=0 "
            f"schedule={total} steps ema=0.99") in r.stdout.splitlines()
    ema_ckpt = tmp_path / "net_ema.pth"
    assert ckpt.exists() and ema_ckpt.exists()
    main, avg = torch.load(ckpt), torch.load(ema_ckpt)
    assert list(main) == list(avg)
    assert all(main[k].shape == avg[k].shape for k in main)
    assert any(not torch.equal(main[k], avg[k]) for k in main)


@pytest.mark.parametrize("script", ["serial", "ddp"])
def test_scripts_without_the_knobs_are_as_before(tmp_path, script):
    ckpt = tmp_path / "net.pth"
    cmd = SERIAL if script == "serial" else _ddp(29744)
    r = _run(cmd, dict(KNOBS, MI355X_CKPT=str(ckpt)))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Finished Training (3 steps" in r.stdout
    assert _ema_lines(r) == []
    assert "optimizer:" not in r.stdout
    assert ckpt.exists()
    assert [p.name for p in tmp_path.iterdir()] == ["net.pth"]
