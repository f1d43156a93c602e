"""The lars.hip kernels on hardware: per-tensor norms against fp64 on a
table of misaligned tensors, three steps against the CPU fallback and a
per-tensor fp64 reference, untouched neighbours, run-to-run determinism, the
non-finite flag in head, body and tail, real train steps of Net and
ResNet-18, and a captured fp16 step that follows a device-side learning
rate and skips an overflowing replay.

Observed on an MI355X, next to each bound (more in profiles/r09_lars.md):
  per-tensor and global norms, bound max(4 x torch's fp32 error, 8 * 2^-24
    = 4.77e-07) relative: at most 8.1e-08 on the table (torch 7.0e-08),
    4.0e-08 / 2.5e-08 for |w| / |g| of the 2 097 159-element tensor
  three steps, rtol 1e-5 / atol 1e-6: max |w - fp64| 3.8e-07, max |m - fp64|
    4.1e-07, max |w - CPU fallback| 4.8e-07
  trust ratios, bound 32 * 2^-24 = 1.91e-06 relative: 2.0e-07 against fp64
    and 1.2e-07 against the fallback on the table, 2.7e-07 for Net,
    1.9e-07 for ResNet-18
  all tensors excluded against sgd_step, rtol 1e-6: 0 (bit-identical with
    this compiler's contraction of sgd_kernel; not asserted)
  real train steps, rtol 1e-5 / atol 1e-6: max |w - fp64| 3.9e-09 (Net),
    6.0e-08 (ResNet-18); max |m - fp64| 8.9e-09
"""

import pytest
import torch

from _lars_common import (EXCLUDE, HP, SIZES, TILE, ULP8, ZERO_G, ZERO_W,
                          assert_trust, offsets_of, ref_step, ref_trajectory,
                          spans, synthetic)
from mi355x import amp, ops, optim
from mi355x.models import Net, build_model
from mi355x.ops import cross_entropy
from mi355x.ops import functional as fn
from mi355x.parallel.flat import FlatState

pytestmark = pytest.mark.gpu

OFF = offsets_of(SIZES)
REF_KW = dict(lr=HP["lr"], mu=HP["mu"], wd=HP["wd"], eta=HP["eta"],
              eps=HP["eps"], grad_scale=HP["grad_scale"])
BIG_SIZES = [2 ** 21 + 7, 5]     # 513 tiles of one tensor, then a tiny one


def _stats(w, g, plan, st):
    return ops.lars_stats(w, g, plan, st, HP["grad_scale"], float("inf"),
                          HP["wd"], HP["eta"], HP["eps"])


def _step(w, g, m, plan, st, lr=HP["lr"], wd=HP["wd"]):
    ops.lars_stats(w, g, plan, st, HP["grad_scale"], float("inf"), wd,
                   HP["eta"], HP["eps"])
    ops.lars_step(w, g, m, plan, st, lr, HP["mu"], wd, HP["grad_scale"])
    ops.scaler_update(st, HP["grad_scale"])


def _norm_check(got, x, label):
    """max(4 x torch's own fp32 error on the same slice, 8 ulp)."""
    ref = x.double().norm().item()
    if ref == 0.0:
        assert got == 0.0, label
        return
    err = abs(got - ref) / ref
    torch_err = abs(float(torch.linalg.vector_norm(x).item()) - ref) / ref
    bound = max(4 * torch_err, ULP8)
    print(f"{label}: rel err {err:.3e}, torch fp32 {torch_err:.3e}, "
          f"bound {bound:.3e}")
    assert err <= bound, label


@pytest.mark.parametrize("sizes", [SIZES, BIG_SIZES], ids=["table", "large"])
def test_per_tensor_norms_match_fp64(sizes):
    off = offsets_of(sizes)
    w, _, (g,) = synthetic(steps=1, seed=3, sizes=sizes)
    w, g = w.cuda(), g.cuda()
    exclude = EXCLUDE if sizes is SIZES else [False, False]
    plan = ops.lars_plan(off, exclude, "cuda")
    assert plan.table.shape[0] == sum(-(-n // TILE) for n in sizes)
    st = fn.new_guard_state("cuda")
    stats = _stats(w, g, plan, st).cpu()
    assert stats.shape == (len(sizes), 3)
    for s, (a, b) in enumerate(spans(off)):
        _norm_check(float(stats[s, fn.LARS_WNORM]), w[a:b], f"|w_{s}| n={b - a}")
        _norm_check(float(stats[s, fn.LARS_GNORM]), g[a:b], f"|g_{s}| n={b - a}")
    _norm_check(float(st[fn.GS_RAW_NORM]), g, "global |g|")
    assert int(st.view(torch.int32)[fn.GS_NONFINITE]) == 0


def test_three_steps_match_fallback_and_fp64():
    w, m, grads = synthetic()
    ref = ref_trajectory(w, m, grads, OFF, EXCLUDE, **REF_KW)
    wg, mg = w.cuda(), m.cuda()
    plan_g = ops.lars_plan(OFF, EXCLUDE, "cuda")
    plan_c = ops.lars_plan(OFF, EXCLUDE, "cpu")
    st_g, st_c = fn.new_guard_state("cuda"), fn.new_guard_state("cpu")
    for k, g in enumerate(grads):
        _step(wg, g.cuda(), mg, plan_g, st_g)
        _step(w, g, m, plan_c, st_c)
        rw, rm, rt, _ = ref[k]
        trust = plan_g.stats[:, fn.LARS_TRUST].cpu()
        print(f"step {k + 1}: max |w - fp64| "
              f"{(wg.cpu().double() - rw).abs().max():.3e}, max |m - fp64| "
              f"{(mg.cpu().double() - rm).abs().max():.3e}, max |w - cpu| "
              f"{(wg.cpu() - w).abs().max():.3e}")
        for got in (wg.cpu(), w):
            torch.testing.assert_close(got.double(), rw, rtol=1e-5, atol=1e-6)
        for got in (mg.cpu(), m):
            torch.testing.assert_close(got.double(), rm, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(wg.cpu(), w, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(mg.cpu(), m, rtol=1e-5, atol=1e-6)
        assert_trust(trust, rt, f"gpu against fp64, step {k + 1}")
        assert_trust(trust, plan_c.stats[:, fn.LARS_TRUST].double(),
                     f"gpu against fallback, step {k + 1}")
        for s, ex in enumerate(EXCLUDE):
            if ex or s == ZERO_G or (s == ZERO_W and k == 0):
                assert float(trust[s]) == 1.0, (k, s)
            else:
                assert float(trust[s]) != 1.0, (k, s)


def test_neighbours_stay_intact():
    w, m, (g,) = synthetic(steps=1)
    n, pad = OFF[-1], 16
    bufs = []
    for src in (w, g, m):
        b = torch.full((n + 2 * pad,), 12345.0, device="cuda")
        b[pad:pad + n] = src.cuda()
        bufs.append(b)
    views = [b[pad:pad + n] for b in bufs]
    plan = ops.lars_plan(OFF, EXCLUDE, "cuda")
    _step(views[0], views[1], views[2], plan, fn.new_guard_state("cuda"))
    assert not torch.equal(views[0].cpu(), w)
    guard = torch.full((pad,), 12345.0)
    for b in bufs:
        assert torch.equal(b[:pad].cpu(), guard)
        assert torch.equal(b[pad + n:].cpu(), guard)
    assert torch.equal(views[1].cpu(), g)          # the gradient is read only


def test_stats_are_deterministic():
    w, _, (g,) = synthetic(steps=1)
    w, g = w.cuda(), g.cuda()
    plan = ops.lars_plan(OFF, EXCLUDE, "cuda")
    st = fn.new_guard_state("cuda")
    runs = []
    for k in range(3):
        if k == 1:
            plan.slab.fill_(float("nan"))    # stale slab contents: no effect
        if k == 2:
            torch.randn(1 << 20, device="cuda").sum()   # unrelated kernels
        st[fn.GS_NONFINITE:fn.GS_RAW_NORM + 1] = 0
        _stats(w, g, plan, st)
        runs.append((plan.stats.view(torch.int32).cpu().clone(),
                     st.view(torch.int32)[fn.GS_NONFINITE:fn.GS_RAW_NORM + 1]
                     .cpu().clone()))
    assert bool(torch.isfinite(plan.stats).all())
    for stats, out in runs[1:]:
        assert torch.equal(stats, runs[0][0])
        assert torch.equal(out, runs[0][1])


# the first element of a misaligned tensor (scalar head); inside a 16-byte
# vector (tensor 6 starts at 1 modulo 4: head 3, so element 100 is lane
# element 1 of vector 24); a full tile's last element (tensor 7's first
# tile, head 3, 1023 vectors, tail 1: a tail too, followed by a one-element
# tile); and the end of tensor 8 (8191 elements from 2 modulo 4: its last
# tile has head 2, 1023 vectors and a tail of 1)
NF_WHERE = {"head": OFF[1], "body": OFF[5] + 100,
            "tile_end": OFF[6] + TILE - 1, "tail": OFF[8] - 1}


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
@pytest.mark.parametrize("where", list(NF_WHERE))
def test_non_finite_gradient_writes_nothing(bad, where):
    assert OFF[1] % 4 == 1 and OFF[5] % 4 == 1 and OFF[7] % 4 == 2
    w, m, (g,) = synthetic(steps=1)
    g[NF_WHERE[where]] = bad
    wg, mg = w.cuda(), m.cuda()
    plan = ops.lars_plan(OFF, EXCLUDE, "cuda")
    st = fn.new_guard_state("cuda")
    _step(wg, g.cuda(), mg, plan, st)
    ist = st.view(torch.int32)
    assert int(ist[fn.GS_NONFINITE]) == 1
    assert int(ist[fn.GS_SKIPPED]) == 1
    assert torch.equal(wg.cpu(), w) and torch.equal(mg.cpu(), m)


def test_large_finite_values_do_not_raise_the_flag():
    w, m, (g,) = synthetic(steps=1)
    for i in NF_WHERE.values():
        g[i] = 3e38                          # finite; its square is not
    wg, mg = w.cuda(), m.cuda()
    plan = ops.lars_plan(OFF, EXCLUDE, "cuda")
    st = fn.new_guard_state("cuda")
    _step(wg, g.cuda(), mg, plan, st)
    assert int(st.view(torch.int32)[fn.GS_NONFINITE]) == 0
    assert int(st.view(torch.int32)[fn.GS_SKIPPED]) == 0


def test_all_excluded_matches_sgd_step():
    w, m, (g,) = synthetic(steps=1)
    wg, mg, gg = w.cuda(), m.cuda(), g.cuda()
    w2, m2 = wg.clone(), mg.clone()
    plan = ops.lars_plan(OFF, [True] * len(SIZES), "cuda")
    _step(wg, gg, mg, plan, fn.new_guard_state("cuda"))
    # an excluded tensor takes no weight decay
    ops.sgd_step(w2, gg, m2, HP["lr"], HP["mu"], 0.0, HP["grad_scale"])
    assert torch.equal(plan.stats[:, fn.LARS_TRUST].cpu(),
                       torch.ones(len(SIZES)))
    print(f"all excluded against sgd_step: max rel diff w "
          f"{((wg - w2).abs() / w2.abs()).max():.3e}, m "
          f"{((mg - m2).abs() / m2.abs()).max():.3e}")
    torch.testing.assert_close(wg, w2, rtol=1e-6, atol=0)
    torch.testing.assert_close(mg, m2, rtol=1e-6, atol=0)
    assert not torch.equal(wg.cpu(), w)


@pytest.mark.parametrize("model", ["net", "resnet18"])
def test_real_train_steps_match_fp64(model):
    dev = torch.device("cuda")
    torch.manual_seed(0)
    net = (Net() if model == "net" else build_model("resnet18")).to(dev)
    flat = FlatState(net)
    kw = dict(lr=0.1, mu=0.9, wd=5e-4, eta=1e-3, eps=1e-8, grad_scale=1.0)
    opt = optim.LARS(flat, lr=kw["lr"], momentum=kw["mu"],
                     weight_decay=kw["wd"])
    off, exclude = opt.plan.offsets, opt.plan.exclude
    if model == "resnet18":
        assert len(off) - 1 == 62
        assert sum(1 for a in off[:-1] if a % 4) == 61
        assert sum(exclude) == 41
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(16, 3, 32, 32, generator=gen).to(dev)
    y = torch.randint(0, 10, (16,), generator=gen).to(dev)
    for k in range(2):
        opt.zero_grad()
        cross_entropy(net(x), y).backward()
        rw, rm = flat.flat_param.double().cpu(), flat.flat_momentum.double().cpu()
        rt, rnorm = ref_step(rw, rm, flat.flat_grad.double().cpu(), off,
                             exclude, **kw)
        opt.step()
        dw = (flat.flat_param.cpu().double() - rw).abs().max().item()
        dm = (flat.flat_momentum.cpu().double() - rm).abs().max().item()
        print(f"{model} step {k + 1}: max |w - fp64| {dw:.3e}, "
              f"max |m - fp64| {dm:.3e}")
        torch.testing.assert_close(flat.flat_param.cpu().double(), rw,
                                   rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(flat.flat_momentum.cpu().double(), rm,
                                   rtol=1e-5, atol=1e-6)
        trust = opt.last_trust_ratios.cpu()
        assert bool(torch.isfinite(trust).all()) and bool((trust > 0).all())
        assert_trust(trust, rt, f"{model} step {k + 1}")
        assert float(opt.last_grad_norm) == pytest.approx(rnorm, rel=1e-5)
    assert opt.skipped_steps == 0


class _CapturedStep:
    """Net() in fp16, batch 16, one whole train step (zero_grad, forward,
    scaled backward, LARS step with a device-side lr) captured after a
    side-stream warm-up. Build and use inside amp.autocast(torch.float16)."""

    LR = 0.05

    def __init__(self):
        dev = torch.device("cuda")
        torch.manual_seed(0)
        self.net = Net().to(dev)
        self.flat = FlatState(self.net)
        self.lr = torch.tensor(self.LR, device=dev)
        self.opt = optim.LARS(self.flat, lr=self.lr, momentum=0.9,
                              weight_decay=5e-4)
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
        """-> (flat_param, flat_momentum) as they were before the replay."""
        before = self.flat.flat_param.clone(), self.flat.flat_momentum.clone()
        self.graph.replay()
        return before

    def changed(self):
        """-> (weights changed, momentum changed) by one replay."""
        w0, m0 = self.replay()
        return (not torch.equal(w0, self.flat.flat_param),
                not torch.equal(m0, self.flat.flat_momentum))


def test_captured_step_follows_lr_tensor_and_skips_overflow():
    with amp.autocast(torch.float16):
        c = _CapturedStep()
        scaler, opt = c.scaler, c.opt
        for _ in range(2):
            assert c.changed() == (True, True)

        c.lr.fill_(0.0)              # a schedule step between two replays
        assert c.changed() == (False, True)
        c.lr.fill_(c.LR)
        assert c.changed() == (True, True)
        scale0, skipped0 = scaler.scale_value, scaler.skipped_steps
        assert skipped0 == 0

        c.static_x.fill_(float("inf"))
        assert c.changed() == (False, False)
        assert scaler.scale_value == scale0 * 0.5
        assert scaler.skipped_steps == 1 and opt.skipped_steps == 1

        c.static_x.copy_(c.x)
        for _ in range(2):
            assert c.changed() == (True, True)
        assert scaler.scale_value == scale0 * 0.5
        assert scaler.skipped_steps == 1
        assert bool(torch.isfinite(c.static_loss))
        trust = opt.last_trust_ratios
        assert bool(torch.isfinite(trust).all()) and bool((trust > 0).all())
