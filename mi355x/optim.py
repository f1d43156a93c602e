"""Fused SGD with momentum over the flat parameter/grad/momentum buffers.

Semantics of the reference's optim.SGD(lr=0.001, momentum=0.9)
(/root/reference/cifar_example.py:64): v = mu*v + g; p -= lr*v — but as
ONE HIP kernel over the whole flat buffer per step instead of per-tensor
launches. grad_scale folds the DDP 1/world_size average (and the AMP
1/loss_scale) into the same kernel.

Guarded path (max_grad_norm set, or step(scaler=DeviceGradScaler)): one
reduction over flat_grad leaves its norm and inf/nan count on the device,
and the SGD kernel reads them there — global-norm clipping and the
skip-on-overflow decision with no host sync, so the step stays
graph-capturable.

LARS is the large-batch optimizer over the same buffers: per-tensor trust
ratios from a tile reduction that respects tensor boundaries in the flat
layout (mi355x/csrc/lars.hip), always guarded.

LRSchedule and EMA ride on a step clock the optimizer keeps on the device
(layout: mi355x/csrc/gradstat.hip): a count of the steps that were applied,
the learning rate the next one uses and the weight of the next EMA update.
One thread advances it after every step that was not skipped for overflow,
and the update kernels read it, so a captured step follows a warmup/decay
schedule and keeps a weight average with no host work at all.
"""

from __future__ import annotations

import contextlib
import math
import os

import numpy as np
import torch

from mi355x import ops
from mi355x.ops import functional as _fn
from mi355x.parallel.flat import FlatState


class LRSchedule:
    """A learning-rate schedule as a table: ``values`` is a float32 tensor of
    T >= 1 learning rates, and applied step number t (0-based; a step skipped
    for overflow does not count) uses ``values[min(t, T-1)]``. The table is
    evaluated on the host in float64 and rounded to float32 once; the device
    only looks it up, so the lr of every step is the table's to the bit.

    Pass it as ``lr`` to optim.SGD or optim.LARS. Any shape the two builders
    do not cover is a list handed to the constructor."""

    def __init__(self, values, device=None):
        if isinstance(values, torch.Tensor):
            values = values.detach().cpu().double().numpy()
        v = np.asarray(values, dtype=np.float64).reshape(-1)
        if v.size < 1:
            raise ValueError("LRSchedule: needs at least one learning rate")
        if not np.isfinite(v).all():
            raise ValueError("LRSchedule: learning rates must be finite")
        self.values = torch.from_numpy(v.astype(np.float32))
        if device is not None:
            self.values = self.values.to(device)

    def __len__(self):
        return self.values.numel()

    @staticmethod
    def _build(decay, base_lr, warmup_steps, total_steps, end_lr,
               warmup_start, device):
        W, T = int(warmup_steps), int(total_steps)
        if T < 1 or W < 0:
            raise ValueError("LRSchedule: total_steps must be >= 1 and "
                             f"warmup_steps >= 0, got {T} and {W}")
        base_lr, end_lr = float(base_lr), float(end_lr)
        warmup_start = float(warmup_start)
        D = max(1, T - 1 - W)
        out = []
        for t in range(T):
            if t < W:
                out.append(warmup_start + (base_lr - warmup_start) * t / W)
            elif t == W:
                out.append(base_lr)      # p == 0, without end_lr's rounding
            else:
                p = min(1.0, (t - W) / D)
                out.append(end_lr + (base_lr - end_lr) * decay(p))
        return LRSchedule(out, device=device)

    @classmethod
    def warmup_cosine(cls, base_lr, warmup_steps, total_steps, end_lr=0.0,
                      warmup_start=0.0, device=None):
        """``total_steps`` entries: linear from warmup_start to base_lr over
        the first ``warmup_steps``, then half a cosine down to end_lr at the
        last entry. With W = warmup_steps, D = max(1, total_steps - 1 - W),
        p = min(1, (t - W) / D):

            t < W:  warmup_start + (base_lr - warmup_start) * t / W
            else:   end_lr + (base_lr - end_lr) * 0.5 * (1 + cos(pi * p))
        """
        return cls._build(lambda p: 0.5 * (1.0 + math.cos(math.pi * p)),
                          base_lr, warmup_steps, total_steps, end_lr,
                          warmup_start, device)

    @classmethod
    def warmup_poly(cls, base_lr, warmup_steps, total_steps, end_lr=0.0,
                    warmup_start=0.0, power=2.0, device=None):
        """The same warm-up, then polynomial decay (the LARS recipe of You et
        al. 2017): ``end_lr + (base_lr - end_lr) * (1 - p) ** power``."""
        power = float(power)
        return cls._build(lambda p: (1.0 - p) ** power, base_lr,
                          warmup_steps, total_steps, end_lr, warmup_start,
                          device)


class EMA:
    """Exponential moving average of the weights, kept by the optimizer's
    update kernel: right after w is updated, ``e += (1 - d_t) * (w - e)``
    with d_t = decay, or min(decay, (1 + t) / (10 + t)) with ``warmup``, t
    counting applied steps. A step skipped for overflow leaves e alone.

    Pass it as ``ema=`` to optim.SGD or optim.LARS, which binds it to the
    flat buffers: ``flat_ema`` is float32 in the layout of ``flat_param``
    and starts as a copy of it (``buffer``: storage to use instead of
    allocating). Evaluate the average inside ``with ema.swapped():``.

    Only parameters are averaged. BN running statistics are not: the EMA
    weights are evaluated with the live running statistics."""

    def __init__(self, decay: float, warmup: bool = True, buffer=None):
        decay = float(decay)
        if not 0.0 <= decay < 1.0:
            raise ValueError(f"EMA: decay must be in [0, 1), got {decay}")
        self.decay = decay
        self.warmup = bool(warmup)
        self.flat_ema = buffer
        self._flat = None

    def _bind(self, flat):
        if self._flat is not None and self._flat is not flat:
            raise ValueError("EMA: already bound to another optimizer's "
                             "buffers")
        p = flat.flat_param
        if self.flat_ema is None:
            self.flat_ema = torch.empty_like(p)
        elif (self.flat_ema.shape != p.shape or self.flat_ema.dtype != p.dtype
              or self.flat_ema.device != p.device):
            raise ValueError("EMA: buffer must match flat_param's shape, "
                             "dtype and device")
        self.flat_ema.copy_(p)
        self._flat = flat

    def _exchange(self):
        p, e = self._flat.flat_param, self.flat_ema
        with torch.no_grad():
            tmp = p.clone()
            p.copy_(e)
            e.copy_(tmp)
        _fn.bump_cache_epoch()  # the 16-bit weight copies are of the other set

    @contextlib.contextmanager
    def swapped(self):
        """Inside, the model computes with the EMA weights. The contents of
        ``flat_param`` and ``flat_ema`` are exchanged in place (parameters
        are views of flat_param, so no pointer moves) and exchanged back on
        exit. Plain copies: meant for an evaluation, not for every step.
        BN layers use the live running statistics inside as outside."""
        if self._flat is None:
            raise RuntimeError("EMA.swapped: not bound to an optimizer yet")
        self._exchange()
        try:
            yield self
        finally:
            self._exchange()


class _Clocked:
    """What optim.SGD and optim.LARS share: the step clock behind an
    LRSchedule and an EMA, and its part of the checkpoint."""

    def _init_clock(self, lr, ema):
        self.schedule = lr if isinstance(lr, LRSchedule) else None
        self.ema = ema
        self.clock = None
        self.lr = lr
        if self.schedule is None and ema is None:
            return
        dev = self.flat.flat_param.device
        if ema is not None:
            ema._bind(self.flat)
        if self.schedule is not None:
            self._table = self.schedule.values.to(dev)
        else:
            # the clock only counts for the EMA: its lr slot is not read
            self._table = torch.zeros(1, dtype=torch.float32, device=dev)
        self.clock = _fn.new_clock(dev, self._table, *self._ema_args())
        if self.schedule is not None:
            self.lr = self.clock[_fn.CK_LR]  # 0-d view: the kernels read it

    def _ema_args(self):
        return ((self.ema.decay, self.ema.warmup) if self.ema is not None
                else (0.0, False))

    def _ema_kw(self):
        if self.ema is None:
            return {}
        return {"ema": self.ema.flat_ema, "clock": self.clock}

    def _advance_clock(self, state):
        if self.clock is not None:
            ops.clock_advance(self.clock, state, self._table,
                              *self._ema_args())

    @property
    def clock_step(self) -> int:
        """Steps applied so far under a schedule or an EMA (syncs; for logs
        and checkpoints). 0 without either."""
        if self.clock is None:
            return 0
        return int(self.clock.view(torch.int32)[_fn.CK_STEP].item())

    def _clock_state_dict(self):
        sd = {"clock_step": self.clock_step}
        if self.ema is not None:
            sd.update(ema=self.ema.flat_ema, ema_decay=self.ema.decay,
                      ema_warmup=self.ema.warmup)
        return sd

    def _load_lr(self, sd):
        if self.schedule is not None:
            return  # the clock's step decides, not the saved float
        if isinstance(self.lr, torch.Tensor):
            self.lr.fill_(sd["lr"])  # in place: a captured graph keeps it
        else:
            self.lr = sd["lr"]

    def _load_clock(self, sd):
        """In place, so a captured graph keeps its pointers. A checkpoint
        from before the clock existed leaves it at 0 and re-seeds the EMA
        from the parameters as they are now (load the model first)."""
        if self.clock is None:
            return
        if self.ema is not None:
            if "ema" in sd:
                self.ema.flat_ema.copy_(sd["ema"])
                self.ema.decay = float(sd["ema_decay"])
                self.ema.warmup = bool(sd["ema_warmup"])
            else:
                self.ema.flat_ema.copy_(self.flat.flat_param)
        _fn.clock_set(self.clock, sd.get("clock_step", 0), self._table,
                      *self._ema_args())


class SGD(_Clocked):
    """``lr`` is a float or an LRSchedule; with the schedule ``self.lr`` is
    the 0-d device view of the clock's lr slot (``float()`` of it syncs: for
    logs). ``ema`` is an optim.EMA or None. With either, every step takes
    the guarded path (bit-identical to the plain one at loss scale 1 with no
    clipping), which supplies the skip decision the clock needs."""

    def __init__(self, flat: FlatState, lr, momentum: float = 0.0,
                 weight_decay: float = 0.0, grad_scale: float = 1.0,
                 max_grad_norm: float | None = None, ema: EMA | None = None):
        self.flat = flat
        self._init_clock(lr, ema)
        self.momentum = momentum
        self.weight_decay = weight_decay
        self.grad_scale = grad_scale
        self.max_grad_norm = max_grad_norm
        # guarded path only, made on first use: the clip-only guard state
        # (a DeviceGradScaler brings its own) and the reduction's slab
        self._own_state = None
        self._slab = None
        self._guard_state = None  # the state the last guarded step used

    def step(self, scaler=None):
        if (scaler is None and self.max_grad_norm is None
                and self.clock is None):
            ops.sgd_step(self.flat.flat_param, self.flat.flat_grad,
                         self.flat.flat_momentum, self.lr, self.momentum,
                         self.weight_decay, self.grad_scale)
        else:
            self._guarded_step(scaler)
        _fn.bump_cache_epoch()  # invalidate cached 16-bit weight copies

    def _guarded_step(self, scaler):
        g = self.flat.flat_grad
        if scaler is not None:
            state = scaler.state
            dyn = (scaler.growth_factor, scaler.backoff_factor,
                   scaler.growth_interval)
        else:
            if self._own_state is None:
                self._own_state = _fn.new_guard_state(g.device)
            state = self._own_state
            dyn = (1.0, 1.0, 0)  # no loss scale to move
        if g.is_cuda and self._slab is None:
            self._slab = torch.empty(_fn.GRAD_STATS_SLAB, dtype=torch.float32,
                                     device=g.device)
        self._guard_state = state
        max_norm = (float("inf") if self.max_grad_norm is None
                    else float(self.max_grad_norm))
        ops.grad_stats(g, slab=self._slab,
                       out=state[_fn.GS_NONFINITE:_fn.GS_RAW_NORM + 1])
        ops.sgd_step_guarded(self.flat.flat_param, g, self.flat.flat_momentum,
                             state, self.lr, self.momentum, self.weight_decay,
                             self.grad_scale, max_norm, **self._ema_kw())
        ops.scaler_update(state, self.grad_scale, max_norm, *dyn)
        self._advance_clock(state)

    @property
    def last_grad_norm(self):
        """Norm of the true gradient (unscaled, world-averaged) at the last
        guarded step, before clipping: a 0-d device tensor, no sync."""
        if self._guard_state is None:
            raise RuntimeError("last_grad_norm: no guarded step taken yet "
                               "(set max_grad_norm or pass a scaler)")
        return self._guard_state[_fn.GS_LAST_NORM]

    @property
    def skipped_steps(self) -> int:
        """Steps skipped for an inf/nan gradient so far (syncs; for logs)."""
        if self._guard_state is None:
            return 0
        return int(self._guard_state.view(torch.int32)[_fn.GS_SKIPPED].item())

    def zero_grad(self, set_to_none: bool = False):
        self.flat.zero_grad()

    def state_dict(self):
        lr = float(self.lr) if self.schedule is not None else self.lr
        return {"momentum_buffer": self.flat.flat_momentum,
                "lr": lr, "momentum": self.momentum,
                "weight_decay": self.weight_decay,
                "max_grad_norm": self.max_grad_norm,
                **self._clock_state_dict()}

    def load_state_dict(self, sd):
        self.flat.flat_momentum.copy_(sd["momentum_buffer"])
        self._load_lr(sd)
        self.momentum = sd["momentum"]
        self.weight_decay = sd["weight_decay"]
        # absent in checkpoints written before clipping existed
        self.max_grad_norm = sd.get("max_grad_norm", self.max_grad_norm)
        self._load_clock(sd)


class LARS(_Clocked):
    """Layer-wise adaptive rate scaling (You et al. 2017) over the flat
    buffers, for the batch sizes at which one global learning rate stops
    working. Per tensor s, with g the true (unscaled, averaged, clipped)
    gradient:

        trust_s = eta * ||w_s|| / (||g_s|| + wd * ||w_s|| + eps)
        m = mu * m + trust_s * (g + wd * w);   w -= lr * m

    Excluded tensors (default: ndim <= 1, the BN scales/shifts and biases)
    take trust 1 and no weight decay. The adapted gradient goes into the
    same momentum buffer as SGD's and lr multiplies at the end, so lr stays
    a pure schedule knob and checkpoints interchange with optim.SGD.

    Every step is guarded: one pass over the weights and the gradient gives
    the per-tensor norms together with the global norm and the inf/nan
    count (it replaces SGD's grad_stats, the gradient is read once), and the
    update writes nothing on overflow. No host sync; graph-capturable.

    ``lr`` is a float, a 0-d float32 device tensor (a captured step then
    follows ``lr.fill_(v)`` between replays) or an LRSchedule: ``self.lr``
    is then the 0-d view of the step clock's lr slot, which the device
    advances itself. ``ema`` is an optim.EMA or None.
    """

    def __init__(self, flat: FlatState, lr, momentum: float = 0.9,
                 weight_decay: float = 0.0, trust_coefficient: float = 1e-3,
                 eps: float = 1e-8, exclude=None, grad_scale: float = 1.0,
                 max_grad_norm: float | None = None, ema: EMA | None = None):
        self.flat = flat
        self._init_clock(lr, ema)
        self.momentum = momentum
        self.weight_decay = weight_decay
        self.trust_coefficient = trust_coefficient
        self.eps = eps
        self.grad_scale = grad_scale
        self.max_grad_norm = max_grad_norm
        if exclude is None:
            exclude = lambda p: p.ndim <= 1  # noqa: E731
        spans = [flat.offsets[id(p)] for p in flat.params]
        self.plan = ops.lars_plan(
            [0] + [e for _, e in spans], [bool(exclude(p)) for p in flat.params],
            flat.flat_param.device)
        self._own_state = None    # made on first use without a scaler
        self._guard_state = None  # the state the last step used

    def step(self, scaler=None):
        f = self.flat
        if scaler is not None:
            state = scaler.state
            dyn = (scaler.growth_factor, scaler.backoff_factor,
                   scaler.growth_interval)
        else:
            if self._own_state is None:
                self._own_state = _fn.new_guard_state(f.flat_grad.device)
            state = self._own_state
            dyn = (1.0, 1.0, 0)  # no loss scale to move
        self._guard_state = state
        max_norm = (float("inf") if self.max_grad_norm is None
                    else float(self.max_grad_norm))
        ops.lars_stats(f.flat_param, f.flat_grad, self.plan, state,
                       self.grad_scale, max_norm, self.weight_decay,
                       self.trust_coefficient, self.eps)
        ops.lars_step(f.flat_param, f.flat_grad, f.flat_momentum, self.plan,
                      state, self.lr, self.momentum, self.weight_decay,
                      self.grad_scale, max_norm, **self._ema_kw())
        ops.scaler_update(state, self.grad_scale, max_norm, *dyn)
        self._advance_clock(state)
        _fn.bump_cache_epoch()  # invalidate cached 16-bit weight copies

    @property
    def last_trust_ratios(self):
        """trust_s of the last step, one per tensor in flat.params order: a
        device tensor, no sync. All 1 before the first step."""
        return self.plan.stats[:, _fn.LARS_TRUST]

    @property
    def last_grad_norm(self):
        """Norm of the true gradient (unscaled, world-averaged) at the last
        step, before clipping: a 0-d device tensor, no sync."""
        if self._guard_state is None:
            raise RuntimeError("last_grad_norm: no step taken yet")
        return self._guard_state[_fn.GS_LAST_NORM]

    @property
    def skipped_steps(self) -> int:
        """Steps skipped for an inf/nan gradient so far (syncs; for logs)."""
        if self._guard_state is None:
            return 0
        return int(self._guard_state.view(torch.int32)[_fn.GS_SKIPPED].item())

    def zero_grad(self, set_to_none: bool = False):
        self.flat.zero_grad()

    def state_dict(self):
        return {"momentum_buffer": self.flat.flat_momentum,
                "lr": float(self.lr), "momentum": self.momentum,
                "weight_decay": self.weight_decay,
                "max_grad_norm": self.max_grad_norm,
                "trust_coefficient": self.trust_coefficient, "eps": self.eps,
                **self._clock_state_dict()}

    def load_state_dict(self, sd):
        self.flat.flat_momentum.copy_(sd["momentum_buffer"])
        self._load_lr(sd)
        self.momentum = sd["momentum"]
        self.weight_decay = sd["weight_decay"]
        # absent in a checkpoint written by optim.SGD
        self.max_grad_norm = sd.get("max_grad_norm", self.max_grad_norm)
        self.trust_coefficient = sd.get("trust_coefficient",
                                        self.trust_coefficient)
        self.eps = sd.get("eps", self.eps)
        self._load_clock(sd)


def from_env(flat: FlatState, lr, momentum: float = 0.9,
             grad_scale: float = 1.0, max_grad_norm: float | None = None,
             ema: EMA | None = None):
    """The training scripts' optimizer: MI355X_OPTIM=sgd|lars (default sgd),
    MI355X_WD (weight decay, default 0) and, for LARS, MI355X_LARS_ETA (the
    trust coefficient, default 0.001). ``lr`` is a float or an LRSchedule
    (schedule_from_env), ``ema`` an optim.EMA or None (ema_from_env).
    ValueError for any other MI355X_OPTIM."""
    kind = os.environ.get("MI355X_OPTIM", "sgd")
    wd = float(os.environ.get("MI355X_WD", "0"))
    if kind == "sgd":
        return SGD(flat, lr=lr, momentum=momentum, weight_decay=wd,
                   grad_scale=grad_scale, max_grad_norm=max_grad_norm,
                   ema=ema)
    if kind == "lars":
        eta = float(os.environ.get("MI355X_LARS_ETA", "0.001"))
        return LARS(flat, lr=lr, momentum=momentum, weight_decay=wd,
                    trust_coefficient=eta, grad_scale=grad_scale,
                    max_grad_norm=max_grad_norm, ema=ema)
    raise ValueError(f"MI355X_OPTIM={kind}: expected sgd or lars")


def schedule_from_env(lr: float, steps_per_epoch: int, epochs: int):
    """The training scripts' learning rate: ``lr`` itself for
    MI355X_SCHED=const (the default), else an LRSchedule over
    ``epochs * steps_per_epoch`` steps that peaks at ``lr``:
    MI355X_SCHED=cosine|poly with MI355X_WARMUP_EPOCHS (a float, default 0)
    of linear warm-up from 0. ValueError for any other MI355X_SCHED."""
    kind = os.environ.get("MI355X_SCHED", "const")
    warmup_epochs = float(os.environ.get("MI355X_WARMUP_EPOCHS", "0"))
    if kind == "const":
        return lr
    total = max(1, int(epochs) * int(steps_per_epoch))
    warmup = int(round(warmup_epochs * steps_per_epoch))
    if kind == "cosine":
        return LRSchedule.warmup_cosine(lr, warmup, total)
    if kind == "poly":
        return LRSchedule.warmup_poly(lr, warmup, total)
    raise ValueError(f"MI355X_SCHED={kind}: expected const, cosine or poly")


def ema_from_env():
    """optim.EMA(MI355X_EMA) with the warm-up, or None when MI355X_EMA is
    unset or 0."""
    decay = float(os.environ.get("MI355X_EMA", "0"))
    return EMA(decay) if decay else None


def describe(opt) -> str:
    """One line for a training log: the optimizer and what it was built
    with."""
    s = (f"{type(opt).__name__} lr={float(opt.lr):g} "
         f"momentum={opt.momentum:g} weight_decay={opt.weight_decay:g}")
    if isinstance(opt, LARS):
        s += f" trust_coefficient={opt.trust_coefficient:g}"
    # under a schedule lr above is the next step's (float() of it syncs)
    if getattr(opt, "schedule", None) is not None:
        s += f" schedule={len(opt.schedule)} steps"
    if getattr(opt, "ema", None) is not None:
        s += f" ema={opt.ema.decay:g}"
    return s
