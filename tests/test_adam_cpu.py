"""optim.AdamW / optim.LAMB and the plain-torch twins of ops.adam_step /
ops.lamb_step on the CPU: three steps against float64 at the GPU test's
tolerances, a checkpoint round trip, and from_env."""

import pytest
import torch

from _adam_common import CASES, compare, make, reference, run, start
from _lars_common import EXCLUDE, ZERO_G, ZERO_W
from mi355x import optim


@pytest.mark.parametrize("case", list(CASES))
def test_three_steps_match_fp64(case):
    kind, max_norm, wd, exclude = CASES[case]
    w0, grads = start()
    ref = reference(kind, w0, grads, max_norm, wd, exclude)
    opt = make(kind, w0, "cpu", max_norm, wd, exclude)
    for k, got in enumerate(run(opt, grads)):
        compare(got, ref[k], f"{case} step {k + 1}")
        if kind == "lamb":
            one = [s for s, ex in enumerate(EXCLUDE) if ex]
            one += [ZERO_W] if k == 0 else []
            one += [ZERO_G] if wd == 0.0 else []
            assert [s for s, t in enumerate(got[3]) if t == 1.0] == sorted(one)
    assert opt.clock_step == 3 and opt.skipped_steps == 0


@pytest.mark.parametrize("kind", ["adamw", "lamb"])
def test_state_dict_round_trip_continues_bit_identically(kind):
    w0, grads = start()
    kw = dict(max_norm=1.0, wd=1e-2, exclude=EXCLUDE)
    sched = [1e-2, 2e-2, 5e-3]
    a = make(kind, w0, "cpu", ema=optim.EMA(0.9), **kw)
    a.lr = 3e-3                      # a float lr travels with the checkpoint
    run(a, grads[:2])
    sd = {k: v.clone() if isinstance(v, torch.Tensor) else v
          for k, v in a.state_dict().items()}
    assert {"exp_avg", "exp_avg_sq", "lr", "betas", "eps", "weight_decay",
            "max_grad_norm", "clock_step", "ema"} <= set(sd)
    b = make(kind, a.flat.flat_param.clone(), "cpu", ema=optim.EMA(0.5), **kw)
    ptrs = [t.data_ptr() for t in (b.flat.flat_momentum, b.exp_avg_sq, b.clock)]
    b.load_state_dict(sd)
    assert ptrs == [t.data_ptr() for t in (b.flat.flat_momentum, b.exp_avg_sq,
                                           b.clock)]
    assert b.lr == 3e-3 and b.clock_step == 2 and b.ema.decay == 0.9
    (sa,), (sb,) = run(a, grads[2:]), run(b, grads[2:])
    for x, y in zip(sa, sb):
        assert x is None or torch.equal(x, y)
    assert torch.equal(a.ema.flat_ema, b.ema.flat_ema)
    # under a schedule the clock's step decides the lr, not the saved float
    c = make(kind, w0, "cpu", **dict(kw, lr=optim.LRSchedule(sched)))
    c.load_state_dict(sd)
    assert float(c.lr) == pytest.approx(sched[2])


@pytest.mark.parametrize("kind", ["adamw", "lamb"])
def test_from_env_builds_the_adaptive_optimizers(kind, monkeypatch):
    w0, _ = start(steps=1)
    flat = make(kind, w0, "cpu", None, 0.0, EXCLUDE).flat
    monkeypatch.setenv("MI355X_OPTIM", kind)
    monkeypatch.setenv("MI355X_WD", "0.05")
    opt = optim.from_env(flat, lr=1e-3, momentum=0.5, max_grad_norm=2.0)
    assert type(opt) is {"adamw": optim.AdamW, "lamb": optim.LAMB}[kind]
    assert (opt.betas, opt.weight_decay, opt.max_grad_norm) == (
        (0.9, 0.999), 0.05, 2.0)
    assert optim.describe(opt) == (f"{type(opt).__name__} lr=0.001 "
                                   "betas=(0.9, 0.999) eps=1e-08 "
                                   "weight_decay=0.05")
    monkeypatch.setenv("MI355X_BETA1", "0.8")
    monkeypatch.setenv("MI355X_BETA2", "0.99")
    assert optim.from_env(flat, lr=1e-3).betas == (0.8, 0.99)
    monkeypatch.setenv("MI355X_OPTIM", "adam")
    with pytest.raises(ValueError, match="MI355X_OPTIM=adam: expected sgd or "
                                         "lars .*adamw or lamb"):
        optim.from_env(flat, lr=1e-3)
