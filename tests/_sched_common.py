"""Shared by test_sched_cpu.py and test_gpu_sched.py: the flat layout with
sentinels around every buffer, the scripted run (a warmup/cosine schedule,
an EMA, an inf in one gradient, optionally a clipped last step) driven
through optim.SGD / optim.LARS on a chosen device, and the same run as an
explicit fp64 loop (plain torch and math, independent of mi355x.ops)."""

import functools
import math

import numpy as np
import torch

from _lars_common import offsets_of, ref_step as lars_ref_step
from mi355x import optim

# 12,359 elements: no multiple of 4 (the guarded SGD kernel's scalar tail);
# the tensors start at 0, 5, 4104, 4105 and 12295, that is at 0, 1, 0, 1
# and 3 modulo 4, so three of them begin off a 16-byte boundary (LARS tile
# heads of 3, 3 and 1 elements); tensors 1 and 3 span a 4096-element LARS
# tile boundary; tensor 2 is one element
SIZES = [5, 4099, 1, 8190, 64]
OFF = offsets_of(SIZES)
N = OFF[-1]
EXCLUDE = [False, False, True, False, True]     # the 1-D ones, as LARS picks
PAD = 64                                        # keeps 16-byte alignment
SENTINEL = 12345.0

HP = dict(mu=0.9, wd=1e-4, grad_scale=0.5)
LARS_HP = dict(eta=1e-3, eps=1e-8)
DECAY = 0.99
STEPS = 6
INF_STEP = 2                 # 0-based: "step 3"
CLIP_NORM = 0.5              # the optional 7th step clips to this


def schedule():
    """Five entries for six or seven steps: the clamp to the last entry is
    part of the run."""
    return optim.LRSchedule.warmup_cosine(0.1, 2, 5, end_lr=0.001,
                                          warmup_start=0.01)


def inputs(steps=STEPS + 1, seed=5):
    """-> (w0, m0, [g_1..g_steps]) float32 on the CPU; g_3 holds an inf in
    the middle of the 16-byte body of tensor 3."""
    gen = torch.Generator().manual_seed(seed)
    w = torch.randn(N, generator=gen)
    m = torch.randn(N, generator=gen)
    grads = [torch.randn(N, generator=gen) for _ in range(steps)]
    grads[INF_STEP][OFF[3] + 1001] = float("inf")
    return w, m, grads


class PaddedFlat:
    """What the optimizers use of a FlatState, over buffers that carry PAD
    sentinel elements in front and behind."""

    def __init__(self, w, m, device):
        self.whole = {k: torch.full((N + 2 * PAD,), SENTINEL, device=device)
                      for k in ("param", "grad", "momentum", "ema")}
        view = {k: b[PAD:PAD + N] for k, b in self.whole.items()}
        self.flat_param, self.flat_grad = view["param"], view["grad"]
        self.flat_momentum, self.ema_buffer = view["momentum"], view["ema"]
        self.flat_param.copy_(w)
        self.flat_momentum.copy_(m)
        self.flat_grad.zero_()
        self.params, self.offsets = [], {}
        for (a, b), ex in zip(zip(OFF, OFF[1:]), EXCLUDE):
            p = self.flat_param[a:b].view((b - a,) if ex else (b - a, 1))
            self.params.append(p)
            self.offsets[id(p)] = (a, b)

    @property
    def numel(self):
        return N

    def zero_grad(self):
        self.flat_grad.zero_()

    def sentinels_intact(self):
        guard = torch.full((PAD,), SENTINEL)
        return all(torch.equal(b[:PAD].cpu(), guard)
                   and torch.equal(b[PAD + N:].cpu(), guard)
                   for b in self.whole.values())


def build(kind, device, lr=None, ema=True, w=None, m=None):
    """-> (flat, optimizer) on ``device``; lr defaults to schedule()."""
    if w is None:
        w, m, _ = inputs()
    flat = PaddedFlat(w, m, device)
    kw = dict(lr=schedule() if lr is None else lr, momentum=HP["mu"],
              weight_decay=HP["wd"], grad_scale=HP["grad_scale"],
              ema=(optim.EMA(DECAY, warmup=True, buffer=flat.ema_buffer)
                   if ema else None))
    if kind == "sgd":
        return flat, optim.SGD(flat, **kw)
    opt = optim.LARS(flat, trust_coefficient=LARS_HP["eta"],
                     eps=LARS_HP["eps"], **kw)
    assert opt.plan.exclude == EXCLUDE
    return flat, opt


def snapshot(flat, opt):
    """Bit-exact CPU copies of w, m, e and the clock (as int32)."""
    return (flat.flat_param.cpu().clone(), flat.flat_momentum.cpu().clone(),
            opt.ema.flat_ema.cpu().clone() if opt.ema is not None else None,
            opt.clock.view(torch.int32).cpu().clone())


def run(kind, device, clip_last=False):
    """The scripted run -> (flat, opt, [lr each step used],
    [snapshot after each step], [the gradient buffer after each step])."""
    _, _, grads = inputs()
    flat, opt = build(kind, device)
    lrs, snaps, gbufs = [], [snapshot(flat, opt)], []
    for k in range(STEPS + (1 if clip_last else 0)):
        if k == STEPS:
            opt.max_grad_norm = CLIP_NORM
        flat.flat_grad.copy_(grads[k])
        lrs.append(float(opt.lr))
        opt.step()
        snaps.append(snapshot(flat, opt))
        gbufs.append(flat.flat_grad.cpu().clone())
    return flat, opt, lrs, snaps[1:], gbufs


def omd_f64(t, decay=DECAY, warmup=True):
    d = min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay
    return 1.0 - d


@functools.lru_cache(maxsize=None)
def reference(kind, clip_last=False):
    """The same run as an explicit float64 loop -> [(w, m, e, applied steps
    so far) after each step]. Computed once; treat as read-only."""
    w0, m0, grads = inputs()
    table = schedule().values.double().tolist()
    w, m = w0.double().clone(), m0.double().clone()
    e = w.clone()
    t, out = 0, []
    for k in range(STEPS + (1 if clip_last else 0)):
        g = grads[k].double()
        max_norm = CLIP_NORM if k == STEPS else None
        if bool(torch.isfinite(g).all()):
            lr = table[min(t, len(table) - 1)]
            if kind == "lars":
                lars_ref_step(w, m, g, OFF, EXCLUDE, lr=lr, mu=HP["mu"],
                              wd=HP["wd"], grad_scale=HP["grad_scale"],
                              max_norm=max_norm, **LARS_HP)
            else:
                norm = float(g.norm()) * HP["grad_scale"]
                coef = (1.0 if max_norm is None
                        else min(1.0, max_norm / (norm + 1e-6)))
                m.mul_(HP["mu"]).add_(g * (HP["grad_scale"] * coef)
                                      + HP["wd"] * w)
                w.sub_(lr * m)
            e.add_(omd_f64(t) * (w - e))
            t += 1
        out.append((w.clone(), m.clone(), e.clone(), t))
    return out


def f32(x):
    return float(np.float32(x))


def cosine_f64(t, base, W, T, end, start):
    """An evaluation of the builder's formula that shares no code with it."""
    if t < W:
        return start + (base - start) * t / W
    p = min(1.0, (t - W) / max(1, T - 1 - W))
    return end + (base - end) * 0.5 * (1.0 + math.cos(math.pi * p))


def poly_f64(t, base, W, T, end, start, power):
    if t < W:
        return start + (base - start) * t / W
    p = min(1.0, (t - W) / max(1, T - 1 - W))
    return end + (base - end) * (1.0 - p) ** power
