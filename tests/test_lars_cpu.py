"""optim.LARS and the ops.lars_* plain-torch fallbacks on the CPU, against a
per-tensor fp64 reference written in _lars_common.py."""

import pytest
import torch

from _lars_common import (EXCLUDE, HP, SIZES, TRUST_RTOL, ZERO_G, ZERO_W,
                          assert_trust, offsets_of, ref_step, ref_trajectory,
                          synthetic, table_flat)
from mi355x import amp, ops, optim
from mi355x.models import Net
from mi355x.ops import functional as fn
from mi355x.parallel.flat import FlatState

OFF = offsets_of(SIZES)
REF_KW = dict(lr=HP["lr"], mu=HP["mu"], wd=HP["wd"], eta=HP["eta"],
              eps=HP["eps"], grad_scale=HP["grad_scale"])


def _lars(flat, **kw):
    args = dict(lr=HP["lr"], momentum=HP["mu"], weight_decay=HP["wd"],
                trust_coefficient=HP["eta"], eps=HP["eps"],
                grad_scale=HP["grad_scale"])
    args.update(kw)
    return optim.LARS(flat, **args)


def test_fallback_matches_fp64_reference():
    w, m, grads = synthetic()
    ref = ref_trajectory(w, m, grads, OFF, EXCLUDE, **REF_KW)
    plan = ops.lars_plan(OFF, EXCLUDE, "cpu")
    st = fn.new_guard_state("cpu")
    for k, g in enumerate(grads):
        ops.lars_stats(w, g, plan, st, HP["grad_scale"], float("inf"),
                       HP["wd"], HP["eta"], HP["eps"])
        ops.lars_step(w, g, m, plan, st, HP["lr"], HP["mu"], HP["wd"],
                      HP["grad_scale"])
        ops.scaler_update(st, HP["grad_scale"])
        rw, rm, rt, rnorm = ref[k]
        print(f"step {k + 1}: max |dw| {(w.double() - rw).abs().max():.3e}, "
              f"max |dm| {(m.double() - rm).abs().max():.3e}")
        torch.testing.assert_close(w.double(), rw, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(m.double(), rm, rtol=1e-5, atol=1e-6)
        assert_trust(plan.stats[:, fn.LARS_TRUST], rt, f"step {k + 1}")
        assert float(st[fn.GS_LAST_NORM]) == pytest.approx(rnorm, rel=1e-6)


def test_trust_ratios_special_tensors():
    w, m, grads = synthetic(steps=1)
    flat = table_flat(w, m)
    opt = _lars(flat)
    assert opt.plan.exclude == EXCLUDE
    flat.flat_grad.copy_(grads[0])
    opt.step()
    trust = opt.last_trust_ratios
    for s, ex in enumerate(EXCLUDE):
        if ex or s in (ZERO_W, ZERO_G):
            assert float(trust[s]) == 1.0, s
        else:
            assert 0 < float(trust[s]) < 1.0, s
    assert float(opt.plan.stats[ZERO_W, fn.LARS_WNORM]) == 0.0
    assert float(opt.plan.stats[ZERO_G, fn.LARS_GNORM]) == 0.0


def test_excluded_tensors_get_no_weight_decay():
    # zero gradient and momentum: only the decay term can move a weight
    w, _, _ = synthetic(steps=0)
    flat = table_flat(w, torch.zeros_like(w))
    opt = _lars(flat, weight_decay=0.1)
    opt.step()
    for s, (a, b) in enumerate(zip(OFF, OFF[1:])):
        same = torch.equal(flat.flat_param[a:b], w[a:b])
        assert same == (EXCLUDE[s] or s == ZERO_W), s


def test_model_layout_and_exclude_predicate():
    torch.manual_seed(0)
    flat = FlatState(Net())
    opt = optim.LARS(flat, lr=0.1)
    assert len(flat.params) == 10
    assert opt.plan.exclude == [p.ndim <= 1 for p in flat.params]
    assert sum(opt.plan.exclude) == 5
    assert opt.plan.offsets == [0] + [flat.offsets[id(p)][1]
                                      for p in flat.params]
    assert opt.last_trust_ratios.shape == (10,)
    flat.flat_grad.normal_()
    opt.step()
    for p, t in zip(flat.params, opt.last_trust_ratios.tolist()):
        assert (t == 1.0) == (p.ndim <= 1)

    custom = optim.LARS(flat, lr=0.1, exclude=lambda p: p.numel() > 1000)
    assert custom.plan.exclude == [p.numel() > 1000 for p in flat.params]
    assert 0 < sum(custom.plan.exclude) < 10
    custom.step()
    for p, t in zip(flat.params, custom.last_trust_ratios.tolist()):
        assert (t == 1.0) == (p.numel() > 1000)


def test_non_finite_gradient_skips_the_step():
    w, m, grads = synthetic(steps=1)
    flat = table_flat(w, m)
    opt = _lars(flat)
    assert opt.skipped_steps == 0
    flat.flat_grad.copy_(grads[0])
    flat.flat_grad[OFF[6] + 17] = float("inf")
    opt.step()
    assert torch.equal(flat.flat_param, w)
    assert torch.equal(flat.flat_momentum, m)
    assert opt.skipped_steps == 1
    flat.flat_grad.copy_(grads[0])
    opt.step()
    assert opt.skipped_steps == 1
    for a, b in zip(OFF, OFF[1:]):
        assert not torch.equal(flat.flat_param[a:b], w[a:b])


def test_device_grad_scaler_on_cpu():
    w, m, grads = synthetic(steps=1)
    trust = {}
    for scale in (1.0, 256.0):
        flat = table_flat(w, m)
        opt = _lars(flat)
        scaler = amp.DeviceGradScaler(init_scale=scale, device="cpu")
        flat.flat_grad.copy_(grads[0] * scale)
        opt.step(scaler=scaler)
        assert scaler.scale_value == scale and opt.skipped_steps == 0
        trust[scale] = opt.last_trust_ratios.clone().double()
    rel = ((trust[256.0] - trust[1.0]).abs() / trust[1.0]).max().item()
    print(f"trust under loss scale 256 against 1: max rel diff {rel:.3e}")
    assert rel <= TRUST_RTOL

    p0, m0 = flat.flat_param.clone(), flat.flat_momentum.clone()
    flat.flat_grad[OFF[-1] - 1] = float("inf")
    opt.step(scaler=scaler)
    assert scaler.scale_value == 128.0
    assert scaler.skipped_steps == 1 and opt.skipped_steps == 1
    assert torch.equal(flat.flat_param, p0)
    assert torch.equal(flat.flat_momentum, m0)


def test_clipping_uses_the_clipped_gradient():
    w, m, grads = synthetic(steps=1)
    g = grads[0]
    true_norm = g.double().norm().item() * HP["grad_scale"]
    max_norm = 0.25 * true_norm
    flat = table_flat(w, m)
    opt = _lars(flat, max_grad_norm=max_norm)
    flat.flat_grad.copy_(g)
    opt.step()
    rw, rm = w.double().clone(), m.double().clone()
    rt, rnorm = ref_step(rw, rm, g.double(), OFF, EXCLUDE, max_norm=max_norm,
                         **REF_KW)
    assert float(opt.last_grad_norm) == pytest.approx(true_norm, rel=1e-6)
    assert rnorm == pytest.approx(true_norm, rel=1e-12)
    torch.testing.assert_close(flat.flat_param.double(), rw,
                               rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(flat.flat_momentum.double(), rm,
                               rtol=1e-5, atol=1e-6)
    assert_trust(opt.last_trust_ratios, rt, "clipped")
    # and the clipped trust ratios differ from the unclipped ones
    ut, _ = ref_step(w.double().clone(), m.double().clone(), g.double(), OFF,
                     EXCLUDE, **REF_KW)
    assert float((rt / ut).max()) > 2.0


def test_state_dict_round_trip_and_sgd_interchange():
    w, m, grads = synthetic(steps=1)
    flat = table_flat(w, m)
    opt = _lars(flat, lr=torch.tensor(0.25), max_grad_norm=3.0)
    flat.flat_grad.copy_(grads[0])
    opt.step()
    sd = opt.state_dict()
    assert isinstance(sd["lr"], float) and sd["lr"] == 0.25
    assert torch.equal(sd["momentum_buffer"], flat.flat_momentum)
    saved = {k: (v.clone() if isinstance(v, torch.Tensor) else v)
             for k, v in sd.items()}

    flat2 = table_flat(w, torch.zeros_like(m))
    lr2 = torch.tensor(1.0)
    opt2 = optim.LARS(flat2, lr=lr2)
    opt2.load_state_dict(saved)
    assert torch.equal(flat2.flat_momentum, saved["momentum_buffer"])
    assert opt2.lr is lr2 and float(lr2) == 0.25
    assert opt2.momentum == HP["mu"] and opt2.weight_decay == HP["wd"]
    assert opt2.max_grad_norm == 3.0
    assert opt2.trust_coefficient == HP["eta"]

    flat3 = table_flat(w, torch.zeros_like(m))
    sgd = optim.SGD(flat3, lr=1.0)
    sgd.load_state_dict(saved)
    assert torch.equal(flat3.flat_momentum, saved["momentum_buffer"])
    assert sgd.lr == 0.25 and sgd.momentum == HP["mu"]
    opt2.load_state_dict(sgd.state_dict())       # and back
    assert float(lr2) == 0.25 and opt2.trust_coefficient == HP["eta"]


def test_from_env_builds_what_the_knobs_ask_for(monkeypatch):
    w, m, _ = synthetic(steps=0)
    flat = table_flat(w, m)
    for k in ("MI355X_OPTIM", "MI355X_WD", "MI355X_LARS_ETA"):
        monkeypatch.delenv(k, raising=False)
    opt = optim.from_env(flat, lr=0.3, momentum=0.8, grad_scale=0.25,
                         max_grad_norm=2.0)
    assert type(opt) is optim.SGD
    assert (opt.lr, opt.momentum, opt.weight_decay) == (0.3, 0.8, 0.0)
    assert (opt.grad_scale, opt.max_grad_norm) == (0.25, 2.0)

    monkeypatch.setenv("MI355X_WD", "5e-4")
    opt = optim.from_env(flat, lr=0.3)
    assert type(opt) is optim.SGD and opt.weight_decay == 5e-4
    assert opt.max_grad_norm is None and opt.grad_scale == 1.0
    assert optim.describe(opt) == "SGD lr=0.3 momentum=0.9 weight_decay=0.0005"

    monkeypatch.setenv("MI355X_OPTIM", "lars")
    opt = optim.from_env(flat, lr=0.3, momentum=0.8, grad_scale=0.25,
                         max_grad_norm=2.0)
    assert type(opt) is optim.LARS
    assert (opt.lr, opt.momentum, opt.weight_decay) == (0.3, 0.8, 5e-4)
    assert opt.trust_coefficient == 1e-3
    assert (opt.grad_scale, opt.max_grad_norm) == (0.25, 2.0)

    monkeypatch.setenv("MI355X_LARS_ETA", "0.002")
    opt = optim.from_env(flat, lr=0.3)
    assert type(opt) is optim.LARS and opt.trust_coefficient == 0.002
    assert opt.max_grad_norm is None and opt.grad_scale == 1.0
    assert optim.describe(opt) == ("LARS lr=0.3 momentum=0.9 "
                                   "weight_decay=0.0005 "
                                   "trust_coefficient=0.002")

    monkeypatch.setenv("MI355X_OPTIM", "adam")
    with pytest.raises(ValueError, match="expected sgd or lars"):
        optim.from_env(flat, lr=0.3)


def test_plan_rejects_more_tensors_than_the_kernels_take():
    n = fn.LARS_MAX_TENSORS
    ops.lars_plan(list(range(n + 1)), [False] * n, "cpu")
    with pytest.raises(ValueError, match=str(n)):
        ops.lars_plan(list(range(n + 2)), [False] * (n + 1), "cpu")


def test_argument_validation():
    with pytest.raises(ValueError):
        ops.lars_plan(OFF, EXCLUDE[:-1], "cpu")
    with pytest.raises(ValueError):
        ops.lars_plan([0, 5, 3], [False, False], "cpu")
    plan = ops.lars_plan(OFF, EXCLUDE, "cpu")
    st = fn.new_guard_state("cpu")
    long = torch.zeros(OFF[-1] + 1)
    with pytest.raises(ValueError):
        ops.lars_stats(long, long, plan, st)
    with pytest.raises(ValueError):
        ops.lars_step(long, long, long, plan, st, 0.1, 0.9)
