"""Guarded optimizer step on the CPU fallbacks: global-norm clipping against
torch's clip_grad_norm_, DeviceGradScaler against the host GradScaler, and
the grad_scale (DDP average) folded into the norm. The kernels themselves
are tested in test_gpu_grad_guard.py."""

import math

import pytest
import torch
from torch import nn

from _grad_guard_common import check_trajectory
from mi355x import amp, ops, optim
from mi355x.ops import cross_entropy
from mi355x.ops import functional as fn
from mi355x.parallel.flat import FlatState


def _mlp():
    return nn.Sequential(nn.Linear(8, 16), nn.ReLU(), nn.Linear(16, 10))


@pytest.mark.parametrize("c,clips", [(0.05, True), (1e3, False)])
def test_clipping_matches_torch(c, clips):
    torch.manual_seed(3)
    net_a = _mlp()
    net_b = _mlp()
    net_b.load_state_dict(net_a.state_dict())
    flat = FlatState(net_a)
    opt_a = optim.SGD(flat, lr=0.1, momentum=0.9, weight_decay=1e-4,
                      max_grad_norm=c)
    opt_b = torch.optim.SGD(net_b.parameters(), lr=0.1, momentum=0.9,
                            weight_decay=1e-4)
    x = torch.randn(8, 8)
    y = torch.randint(0, 10, (8,))
    for _ in range(5):
        opt_a.zero_grad()
        cross_entropy(net_a(x), y).backward()
        opt_a.step()
        opt_b.zero_grad()
        torch.nn.functional.cross_entropy(net_b(x), y).backward()
        total = torch.nn.utils.clip_grad_norm_(net_b.parameters(), c)
        opt_b.step()
        # the case does what its name says, at every step
        assert (float(total) > c) == clips
        torch.testing.assert_close(opt_a.last_grad_norm, total,
                                   rtol=1e-5, atol=0)
    assert opt_a.skipped_steps == 0
    for pa, pb in zip(net_a.parameters(), net_b.parameters()):
        torch.testing.assert_close(pa, pb, rtol=1e-4, atol=1e-6)


def test_device_scaler_trajectory_matches_grad_scaler():
    check_trajectory(torch.device("cpu"))


def test_grad_scale_folds_into_norm():
    torch.manual_seed(4)
    flat = FlatState(_mlp())
    opt = optim.SGD(flat, lr=0.1, grad_scale=1 / 4, max_grad_norm=1e9)
    flat.flat_grad.copy_(torch.randn(flat.numel))
    opt.step()
    want = (flat.flat_grad.double() / 4).norm()
    raw = flat.flat_grad.double().norm()
    assert opt.last_grad_norm.dim() == 0
    torch.testing.assert_close(opt.last_grad_norm.double(), want,
                               rtol=1e-6, atol=0)
    assert abs(float(opt.last_grad_norm) - float(raw)) > 0.5 * float(raw)


def test_scaler_and_clipping_norm_is_of_the_unscaled_gradient():
    torch.manual_seed(5)
    flat = FlatState(_mlp())
    opt = optim.SGD(flat, lr=0.1, grad_scale=1 / 2, max_grad_norm=0.5)
    scaler = amp.DeviceGradScaler(init_scale=2.0 ** 8, device="cpu")
    g = torch.randn(flat.numel)
    flat.flat_grad.copy_(scaler.scale(g))
    p0 = flat.flat_param.clone()
    opt.step(scaler=scaler)
    norm = float((g.double() / 2).norm())
    torch.testing.assert_close(float(opt.last_grad_norm), norm,
                               rtol=1e-6, atol=0)
    coef = min(1.0, 0.5 / (norm + 1e-6))
    assert coef < 1.0
    torch.testing.assert_close(flat.flat_param, p0 - 0.1 * (g / 2) * coef,
                               rtol=1e-5, atol=1e-7)


def test_inactive_guard_equals_sgd_step_bitwise():
    g = torch.Generator().manual_seed(8)
    n = 4099
    p, grad, m = (torch.randn(n, generator=g) for _ in range(3))
    p2, m2 = p.clone(), m.clone()
    state = fn.new_guard_state("cpu")
    ops.grad_stats(grad, out=state[fn.GS_NONFINITE:fn.GS_RAW_NORM + 1])
    ops.sgd_step_guarded(p, grad, m, state, 0.1, 0.9, 1e-4, 0.5)
    ops.sgd_step(p2, grad, m2, 0.1, 0.9, 1e-4, 0.5)
    assert torch.equal(p, p2) and torch.equal(m, m2)


def test_grad_stats_fallback():
    g = torch.tensor([3.0, 4.0, 3e38])
    norm, count = ops.grad_stats(g[:2])
    assert float(norm) == 5.0 and int(count) == 0
    norm, count = ops.grad_stats(g)          # finite, though 3e38^2 is not
    assert int(count) == 0
    for bad in (float("inf"), float("-inf"), float("nan")):
        h = g.clone()
        h[1] = bad
        assert int(ops.grad_stats(h)[1]) == 1


def test_clip_only_skips_non_finite_gradient():
    flat = FlatState(_mlp())
    opt = optim.SGD(flat, lr=0.1, momentum=0.9, max_grad_norm=1.0)
    flat.flat_grad.fill_(1.0)
    flat.flat_grad[7] = float("nan")
    p0, m0 = flat.flat_param.clone(), flat.flat_momentum.clone()
    opt.step()
    assert torch.equal(flat.flat_param, p0)
    assert torch.equal(flat.flat_momentum, m0)
    assert opt.skipped_steps == 1


def test_state_dicts_round_trip():
    flat = FlatState(_mlp())
    opt = optim.SGD(flat, lr=0.1, max_grad_norm=2.5)
    sd = opt.state_dict()
    assert sd["max_grad_norm"] == 2.5
    opt2 = optim.SGD(flat, lr=0.3)
    opt2.load_state_dict(sd)
    assert opt2.max_grad_norm == 2.5 and opt2.lr == 0.1

    s = amp.DeviceGradScaler(init_scale=64.0, growth_interval=2, device="cpu")
    flat.flat_grad.fill_(float("inf"))
    opt.step(scaler=s)                       # 32, skipped 1
    flat.flat_grad.zero_()
    opt.step(scaler=s)                       # tracker 1
    s2 = amp.DeviceGradScaler(device="cpu")
    s2.load_state_dict(s.state_dict())
    assert s2.scale_value == 32.0 and s2.skipped_steps == 1
    assert s2.growth_interval == 2
    opt.step(scaler=s2)                      # tracker 2 -> grow
    assert s2.scale_value == 64.0
    assert math.isclose(float(s2.state[fn.GS_INV_SCALE]), 1 / 64.0)
