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
"""

from __future__ import annotations

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
