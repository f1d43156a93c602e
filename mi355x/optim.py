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
"""

from __future__ import annotations

import os

import torch

from mi355x import ops
from mi355x.ops import functional as _fn
from mi355x.parallel.flat import FlatState


class SGD:
    def __init__(self, flat: FlatState, lr: float, momentum: float = 0.0,
                 weight_decay: float = 0.0, grad_scale: float = 1.0,
                 max_grad_norm: float | None = None):
        self.flat = flat
        self.lr = lr
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
        if scaler is None and self.max_grad_norm is None:
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
                             self.grad_scale, max_norm)
        ops.scaler_update(state, self.grad_scale, max_norm, *dyn)

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
        return {"momentum_buffer": self.flat.flat_momentum,
                "lr": self.lr, "momentum": self.momentum,
                "weight_decay": self.weight_decay,
                "max_grad_norm": self.max_grad_norm}

    def load_state_dict(self, sd):
        self.flat.flat_momentum.copy_(sd["momentum_buffer"])
        self.lr = sd["lr"]
        self.momentum = sd["momentum"]
        self.weight_decay = sd["weight_decay"]
        # absent in checkpoints written before clipping existed
        self.max_grad_norm = sd.get("max_grad_norm", self.max_grad_norm)


class LARS:
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

    ``lr`` is a float or a 0-d float32 device tensor; with the tensor a
    captured step follows ``lr.fill_(v)`` between replays.
    """

    def __init__(self, flat: FlatState, lr, momentum: float = 0.9,
                 weight_decay: float = 0.0, trust_coefficient: float = 1e-3,
                 eps: float = 1e-8, exclude=None, grad_scale: float = 1.0,
                 max_grad_norm: float | None = None):
        self.flat = flat
        self.lr = lr
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
                      self.grad_scale, max_norm)
        ops.scaler_update(state, self.grad_scale, max_norm, *dyn)
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
                "trust_coefficient": self.trust_coefficient, "eps": self.eps}

    def load_state_dict(self, sd):
        self.flat.flat_momentum.copy_(sd["momentum_buffer"])
        if isinstance(self.lr, torch.Tensor):
            self.lr.fill_(sd["lr"])  # in place: a captured graph keeps it
        else:
            self.lr = sd["lr"]
        self.momentum = sd["momentum"]
        self.weight_decay = sd["weight_decay"]
        # absent in a checkpoint written by optim.SGD
        self.max_grad_norm = sd.get("max_grad_norm", self.max_grad_norm)
        self.trust_coefficient = sd.get("trust_coefficient",
                                        self.trust_coefficient)
        self.eps = sd.get("eps", self.eps)


def from_env(flat: FlatState, lr, momentum: float = 0.9,
             grad_scale: float = 1.0, max_grad_norm: float | None = None):
    """The training scripts' optimizer: MI355X_OPTIM=sgd|lars (default sgd),
    MI355X_WD (weight decay, default 0) and, for LARS, MI355X_LARS_ETA (the
    trust coefficient, default 0.001). ValueError for any other
    MI355X_OPTIM."""
    kind = os.environ.get("MI355X_OPTIM", "sgd")
    wd = float(os.environ.get("MI355X_WD", "0"))
    if kind == "sgd":
        return SGD(flat, lr=lr, momentum=momentum, weight_decay=wd,
                   grad_scale=grad_scale, max_grad_norm=max_grad_norm)
    if kind == "lars":
        eta = float(os.environ.get("MI355X_LARS_ETA", "0.001"))
        return LARS(flat, lr=lr, momentum=momentum, weight_decay=wd,
                    trust_coefficient=eta, grad_scale=grad_scale,
                    max_grad_norm=max_grad_norm)
    raise ValueError(f"MI355X_OPTIM={kind}: expected sgd or lars")


def describe(opt) -> str:
    """One line for a training log: the optimizer and what it was built
    with."""
    s = (f"{type(opt).__name__} lr={float(opt.lr):g} "
         f"momentum={opt.momentum:g} weight_decay={opt.weight_decay:g}")
    if isinstance(opt, LARS):
        s += f" trust_coefficient={opt.trust_coefficient:g}"
    return s
