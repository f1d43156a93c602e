"""Shared by test_grad_guard_cpu.py and test_gpu_grad_guard.py: the scripted
12-step loss-scaling run, driven once through the host GradScaler and once
through DeviceGradScaler on a chosen device."""

import torch
from torch import nn

from mi355x import amp, optim
from mi355x.parallel.flat import FlatState

STEPS = 12
INF_STEPS = (2, 3, 9)      # 0-based steps whose grad buffer gets an inf
GROWTH_INTERVAL = 3
INIT_SCALE = 2.0 ** 10
# host GradScaler by hand: 2^10 clean, clean, [inf -> 2^9], [inf -> 2^8],
# clean x3 -> 2^9, clean x2, [inf -> 2^8], clean, clean
EXPECTED = [1024.0, 1024.0, 512.0, 256.0, 256.0, 256.0, 512.0, 512.0, 512.0,
            256.0, 256.0, 256.0]


def _setup(device):
    torch.manual_seed(11)
    net = nn.Linear(37, 11).to(device)       # 418 params: vectors + a tail
    flat = FlatState(net)
    opt = optim.SGD(flat, lr=0.1, momentum=0.9, weight_decay=1e-4)
    g = torch.Generator().manual_seed(12)
    grads = [torch.randn(flat.numel, generator=g).to(device)
             for _ in range(STEPS)]
    return flat, opt, grads


def run_host(device):
    """-> (scale after each step, params after each step) with GradScaler."""
    flat, opt, grads = _setup(device)
    scaler = amp.GradScaler(init_scale=INIT_SCALE,
                            growth_interval=GROWTH_INTERVAL)
    scales, params = [], []
    for k in range(STEPS):
        used = scaler.scale_value
        flat.flat_grad.copy_(grads[k] * used)
        if k in INF_STEPS:
            flat.flat_grad[flat.numel // 2] = float("inf")
        if scaler.step_ok(flat.flat_grad):
            opt.grad_scale = 1.0 / used
            opt.step()
        scales.append(scaler.scale_value)
        params.append(flat.flat_param.clone().cpu())
    return scales, params


def run_device(device):
    """The same run with DeviceGradScaler: -> (scales, params, skipped)."""
    flat, opt, grads = _setup(device)
    scaler = amp.DeviceGradScaler(init_scale=INIT_SCALE,
                                  growth_interval=GROWTH_INTERVAL,
                                  device=device)
    scales, params = [], []
    for k in range(STEPS):
        flat.flat_grad.copy_(scaler.scale(grads[k]))
        if k in INF_STEPS:
            flat.flat_grad[flat.numel // 2] = float("inf")
        opt.step(scaler=scaler)
        scales.append(scaler.scale_value)
        params.append(flat.flat_param.clone().cpu())
    return scales, params, scaler.skipped_steps, opt.skipped_steps


def check_trajectory(device):
    h_scales, h_params = run_host(device)
    d_scales, d_params, skipped, opt_skipped = run_device(device)
    assert h_scales == EXPECTED
    assert d_scales == h_scales          # exact: powers of two throughout
    assert skipped == len(INF_STEPS) and opt_skipped == skipped
    for k in range(STEPS):
        prev = d_params[k - 1] if k else None
        if k in INF_STEPS:
            torch.testing.assert_close(d_params[k], prev, rtol=0, atol=0)
        elif prev is not None:
            assert not torch.equal(d_params[k], prev)
        # clean steps apply the same update as the host-scaler path
        torch.testing.assert_close(d_params[k], h_params[k],
                                   rtol=1e-5, atol=1e-6)
