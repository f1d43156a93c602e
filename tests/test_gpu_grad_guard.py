"""The gradstat.hip kernels on hardware: grad_stats against fp64, the
non-finite flag, run-to-run determinism, the guarded SGD step against its
CPU fallback and against sgd_step, DeviceGradScaler against the host
GradScaler, and a captured fp16 train step that skips an overflowing replay
on the device.

Observed on an MI355X (relative error of the norm against fp64; the bound
is max(4 x torch's own fp32 error on the same buffer, 8 * 2^-24)): see
profiles/r07_device_scaler.md.
"""

import pytest
import torch

from _grad_guard_common import check_trajectory
from mi355x import amp, ops, optim
from mi355x.models import Net
from mi355x.ops import cross_entropy
from mi355x.ops import functional as fn
from mi355x.parallel.flat import FlatState

pytestmark = pytest.mark.gpu

N_BIG = 2 * 2**10 * 2**10 + 7   # 2048 blocks x 256 x 4, + one vector, + tail
# floor of the allowed error: 8 fp32 ulps, for one rounding each in the
# square, the block sum, the combine, the sqrt and the cast
ULP8 = 8 * 2.0 ** -24


@pytest.fixture(scope="module")
def big():
    g = torch.Generator().manual_seed(21)
    return torch.randn(N_BIG, generator=g).cuda()


def _buf(n, big):
    return big if n == N_BIG else big[:n].clone()


def _stats_out(state):
    return state[fn.GS_NONFINITE:fn.GS_RAW_NORM + 1]


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, N_BIG])
def test_grad_stats_matches_fp64(n, big):
    g = _buf(n, big)
    ref = g.double().norm().item()
    norm, count = ops.grad_stats(g)
    assert norm.dim() == 0 and norm.dtype == torch.float32
    err = abs(float(norm.item()) - ref) / ref
    torch_err = abs(float(torch.linalg.vector_norm(g).item()) - ref) / ref
    bound = max(4 * torch_err, ULP8)
    print(f"grad_stats n={n}: rel err {err:.3e}, torch fp32 {torch_err:.3e}, "
          f"bound {bound:.3e}")
    assert int(count.item()) == 0
    assert err <= bound


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_non_finite_flag(bad, where, big):
    n = 4099                      # index n-1 sits in the scalar tail
    g = big[:n].clone()
    g[{"first": 0, "middle": n // 2, "last": n - 1}[where]] = bad
    _, count = ops.grad_stats(g)
    assert int(count.item()) == 1


def test_non_finite_flag_second_sweep_and_tail(big):
    g = big.clone()
    g[N_BIG - 1] = float("nan")              # tail of the second sweep
    g[2048 * 1024 + 2] = float("inf")        # the extra vector
    _, count = ops.grad_stats(g)
    assert int(count.item()) == 2


def test_large_finite_values_do_not_raise_the_flag(big):
    n = 4099
    g = big[:n].clone()
    for i in (0, n // 2, n - 1):
        g[i] = 3e38                          # finite; its square is not
    assert bool(torch.isfinite(g).all())
    _, count = ops.grad_stats(g)
    assert int(count.item()) == 0


def test_grad_stats_is_deterministic(big):
    slab = torch.full((fn.GRAD_STATS_SLAB,), float("nan"), device="cuda")
    a, _ = ops.grad_stats(big)
    b, _ = ops.grad_stats(big, slab=slab)    # stale slab contents: no effect
    c, _ = ops.grad_stats(big, slab=slab)
    ai, bi, ci = (t.view(torch.int32).item() for t in (a, b, c))
    assert ai == bi == ci


def _guarded(p, grad, m, scale, max_norm):
    st = fn.new_guard_state(p.device, scale=scale)
    ops.grad_stats(grad, out=_stats_out(st))
    ops.sgd_step_guarded(p, grad, m, st, 0.1, 0.9, 1e-4, 0.5, max_norm)
    ops.scaler_update(st, 0.5, max_norm, 2.0, 0.5, 1000)
    return st


@pytest.mark.parametrize("n", [5, 4099])
@pytest.mark.parametrize("scale", [1.0, 256.0])
def test_guarded_sgd_matches_fallback(n, scale):
    g = torch.Generator().manual_seed(8)
    p, grad, m = (torch.randn(n, generator=g) for _ in range(3))
    grad *= scale
    max_norm = 0.25               # true norm ~ 0.5*sqrt(n) >= 1.1: clips
    pg, gg, mg = p.cuda(), grad.cuda(), m.cuda()
    st_gpu = _guarded(pg, gg, mg, scale, max_norm)
    st = _guarded(p, grad, m, scale, max_norm)
    assert float(st[fn.GS_LAST_COEF]) < 1.0
    torch.testing.assert_close(pg.cpu(), p, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(mg.cpu(), m, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(st_gpu.cpu()[fn.GS_RAW_NORM:],
                               st[fn.GS_RAW_NORM:], rtol=1e-6, atol=0)
    assert torch.equal(st_gpu.cpu().view(torch.int32)[:fn.GS_RAW_NORM],
                       st.view(torch.int32)[:fn.GS_RAW_NORM])


@pytest.mark.parametrize("n", [5, 4099, 10001])
def test_inactive_guard_equals_sgd_step_bitwise(n):
    g = torch.Generator().manual_seed(9)
    p, grad, m = (torch.randn(n, generator=g).cuda() for _ in range(3))
    p2, m2 = p.clone(), m.clone()
    st = fn.new_guard_state("cuda")
    ops.grad_stats(grad, out=_stats_out(st))
    ops.sgd_step_guarded(p, grad, m, st, 0.1, 0.9, 1e-4, 0.5, float("inf"))
    ops.sgd_step(p2, grad, m2, 0.1, 0.9, 1e-4, 0.5)
    assert torch.equal(p, p2) and torch.equal(m, m2)
    assert not torch.equal(p, torch.zeros_like(p))


@pytest.mark.parametrize("with_scaler", [False, True])
def test_non_finite_gradient_skips_the_step(with_scaler):
    torch.manual_seed(0)
    flat = FlatState(torch.nn.Linear(64, 65).cuda())   # 4225: vectors + tail
    opt = optim.SGD(flat, lr=0.1, momentum=0.9, weight_decay=1e-4,
                    max_grad_norm=None if with_scaler else 1.0)
    scaler = (amp.DeviceGradScaler(init_scale=1024.0, device="cuda")
              if with_scaler else None)
    flat.flat_momentum.normal_()
    flat.flat_grad.normal_()
    flat.flat_grad[flat.numel - 1] = float("inf")
    p0, m0 = flat.flat_param.clone(), flat.flat_momentum.clone()
    opt.step(scaler=scaler)
    assert torch.equal(flat.flat_param, p0)
    assert torch.equal(flat.flat_momentum, m0)
    assert opt.skipped_steps == 1
    if with_scaler:
        assert scaler.scale_value == 512.0 and scaler.skipped_steps == 1
    flat.flat_grad[flat.numel - 1] = 0.0
    opt.step(scaler=scaler)                            # and then it moves
    assert not torch.equal(flat.flat_param, p0)
    assert opt.skipped_steps == 1


def test_device_scaler_trajectory_matches_grad_scaler():
    check_trajectory(torch.device("cuda"))


class _CapturedStep:
    """Net() in fp16, batch 16, one whole train step (zero_grad, forward,
    scaled backward, guarded optimizer step) captured after a side-stream
    warm-up. Build and use inside amp.autocast(torch.float16)."""

    def __init__(self):
        dev = torch.device("cuda")
        torch.manual_seed(0)
        self.net = Net().to(dev)
        self.flat = FlatState(self.net)
        self.opt = optim.SGD(self.flat, lr=0.05, momentum=0.9)
        self.scaler = amp.DeviceGradScaler(init_scale=2.0 ** 10, device=dev)
        g = torch.Generator().manual_seed(0)
        self.x = torch.randn(16, 3, 32, 32, generator=g).to(dev)
        y = torch.randint(0, 10, (16,), generator=g).to(dev)
        self.static_x, self.static_y = self.x.clone(), y.clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):
                self._step()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.static_loss = self._step()

    def _step(self):
        self.opt.zero_grad()
        loss = cross_entropy(self.net(self.static_x), self.static_y)
        self.scaler.scale(loss).backward()
        self.opt.step(scaler=self.scaler)
        return loss

    def replay(self):
        """-> flat_param as it was before the replay."""
        before = self.flat.flat_param.clone()
        self.graph.replay()
        return before

    def changed(self):
        return not torch.equal(self.replay(), self.flat.flat_param)

    def loss_is_finite(self):
        return bool(torch.isfinite(self.static_loss))


def test_captured_step_skips_overflow_on_device():
    """An all-inf image batch copied into the static input of replay 3
    makes that replay, and only that one, skip. The forward pass turns the
    inf into NaN in conv1; the fused ReLU epilogues keep a NaN (relu_f in
    common.h, test_gpu_relu_nan.py), so it reaches the loss and the whole
    gradient, where grad_stats counts it."""
    with amp.autocast(torch.float16):
        c = _CapturedStep()
        scaler, opt, flat = c.scaler, c.opt, c.flat
        for _ in range(2):                               # replays 1, 2
            assert c.changed()
        scale0, skipped0 = scaler.scale_value, scaler.skipped_steps
        assert skipped0 == 0

        c.static_x.fill_(float("inf"))                   # replay 3
        before = c.replay()
        ist = scaler.state.view(torch.int32)
        print(f"inf-input replay: non-finite count "
              f"{int(ist[fn.GS_NONFINITE].item())}, scale "
              f"{scaler.scale_value}, skipped {scaler.skipped_steps}, "
              f"max |dp| {float((flat.flat_param - before).abs().max()):.3e}")
        assert torch.equal(before, flat.flat_param)
        assert scaler.scale_value == scale0 * 0.5
        assert scaler.skipped_steps == skipped0 + 1
        assert opt.skipped_steps == skipped0 + 1

        c.static_x.copy_(c.x)
        for _ in range(3):                               # replays 4..6
            assert c.changed()
        assert scaler.scale_value == scale0 * 0.5
        assert scaler.skipped_steps == skipped0 + 1
        assert c.loss_is_finite()


def test_captured_step_skips_scale_overflow_on_device():
    """One captured graph, a skip decision per replay: a loss scale of 2^40
    (set in place in the scaler's device state between replays) overflows
    the fp16 backward, as in test_fp16_dynamic_scaling_overflow_recovery.
    Those replays leave the parameters bit for bit alone, halve the scale
    and count a skip; with a workable scale the same graph trains again."""
    with amp.autocast(torch.float16):
        c = _CapturedStep()
        scaler, opt, flat = c.scaler, c.opt, c.flat
        for _ in range(2):
            assert c.changed()
        assert scaler.skipped_steps == 0

        sd = scaler.state_dict()
        scaler.load_state_dict(dict(sd, scale=2.0 ** 40))
        for k in (1, 2):
            assert not c.changed()
            assert scaler.scale_value == 2.0 ** (40 - k)
            assert scaler.skipped_steps == k and opt.skipped_steps == k
        assert not bool(torch.isfinite(opt.last_grad_norm))

        scaler.load_state_dict(dict(scaler.state_dict(), scale=2.0 ** 10))
        for _ in range(3):
            assert c.changed()
        assert scaler.scale_value == 2.0 ** 10
        assert scaler.skipped_steps == 2
        assert c.loss_is_finite()
        assert bool(torch.isfinite(opt.last_grad_norm))


