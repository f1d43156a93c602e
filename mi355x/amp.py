"""Mixed-precision policy for the mi355x kernels.

Compute dtype is bf16 by default (MFMA bf16 peak ~2.5 PF dense on MI355X).
An `autocast(fp16)` context switches the 16-bit kernel dtype to fp16 and —
because fp16 has a narrow exponent — pairs with `GradScaler` loss scaling
(BASELINE config 5: "ResNet-18 AMP fp16 + SyncBatchNorm").

The scaler works on the FLAT fp32 gradient buffer maintained by
mi355x.parallel.flat (one inf/nan scan kernel over the whole buffer,
after the reducer's all-reduce — SURVEY.md §7 hard-part 4).
"""

from __future__ import annotations

import contextlib

import torch

_COMPUTE_DTYPE = torch.bfloat16


def get_compute_dtype() -> torch.dtype:
    return _COMPUTE_DTYPE


def set_compute_dtype(dtype: torch.dtype) -> None:
    global _COMPUTE_DTYPE
    assert dtype in (torch.bfloat16, torch.float16)
    _COMPUTE_DTYPE = dtype


@contextlib.contextmanager
def autocast(dtype: torch.dtype = torch.float16):
    global _COMPUTE_DTYPE
    prev = _COMPUTE_DTYPE
    set_compute_dtype(dtype)
    try:
        yield
    finally:
        _COMPUTE_DTYPE = prev


class GradScaler:
    """Loss scaling for fp16 training over a flat fp32 grad buffer.

    scale() multiplies the loss; after backward + gradient all-reduce the
    caller passes the flat grad buffer to step_ok(), which scans it for
    inf/nan ONCE; if clean, the optimizer consumes grad_scale=1/scale.
    Dynamic scaling: halve on overflow, double every `growth_interval`
    clean steps.
    """

    def __init__(self, init_scale=2.0 ** 14, growth_factor=2.0,
                 backoff_factor=0.5, growth_interval=1000):
        self.scale_value = float(init_scale)
        self.growth_factor = growth_factor
        self.backoff_factor = backoff_factor
        self.growth_interval = growth_interval
        self._clean_steps = 0

    def scale(self, loss: torch.Tensor) -> torch.Tensor:
        return loss * self.scale_value

    def inv_scale(self) -> float:
        return 1.0 / self.scale_value

    def step_ok(self, flat_grad: torch.Tensor) -> bool:
        """True if flat_grad is finite; updates the dynamic scale.

        Callers must capture the scale BEFORE calling (this may grow it):
            used = scaler.scale_value; (loss*used).backward(); ...
            if scaler.step_ok(flat): opt.grad_scale = base/used; opt.step()
        """
        finite = bool(torch.isfinite(flat_grad).all().item())
        if finite:
            self._clean_steps += 1
            if self._clean_steps >= self.growth_interval:
                self.scale_value *= self.growth_factor
                self._clean_steps = 0
        else:
            self.scale_value *= self.backoff_factor
            self._clean_steps = 0
        return finite


class DeviceGradScaler:
    """GradScaler's dynamic loss scaling with the scale, the overflow check
    and the skip decision all on the device: nothing in the step path reads
    a value back, so the whole train step can be captured in a graph.

        optimizer.zero_grad()
        loss = cross_entropy(net(x), y)
        scaler.scale(loss).backward()
        net.finish_grad_sync()          # DDP only
        optimizer.step(scaler=scaler)

    optim.SGD.step(scaler=...) runs the inf/nan scan over the flat grad
    buffer, folds 1/scale into the SGD kernel (which writes nothing on
    overflow) and updates the scale by step_ok's rules, all as kernels on
    the current stream. The optimizer's grad_scale stays the plain DDP
    average; it must not carry 1/scale.

    `state` is the one float32[8] device tensor the kernels share (layout:
    mi355x/csrc/gradstat.hip). `scale_value` and `skipped_steps` sync and
    are for logging.
    """

    def __init__(self, init_scale=2.0 ** 14, growth_factor=2.0,
                 backoff_factor=0.5, growth_interval=1000, device=None):
        from mi355x.ops import functional as _fn
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self._fn = _fn
        self.growth_factor = float(growth_factor)
        self.backoff_factor = float(backoff_factor)
        self.growth_interval = int(growth_interval)
        self.state = _fn.new_guard_state(torch.device(device),
                                         scale=float(init_scale))

    def scale(self, loss: torch.Tensor) -> torch.Tensor:
        return loss * self.state[self._fn.GS_SCALE]

    @property
    def scale_value(self) -> float:
        return float(self.state[self._fn.GS_SCALE].item())

    @property
    def skipped_steps(self) -> int:
        return int(self.state.view(torch.int32)[self._fn.GS_SKIPPED].item())

    def state_dict(self):
        ist = self.state.view(torch.int32)
        return {"scale": self.scale_value,
                "growth_tracker": int(ist[self._fn.GS_TRACKER].item()),
                "skipped_steps": self.skipped_steps,
                "growth_factor": self.growth_factor,
                "backoff_factor": self.backoff_factor,
                "growth_interval": self.growth_interval}

    def load_state_dict(self, sd):
        fn = self._fn
        st = fn.new_guard_state("cpu", scale=float(sd["scale"]))
        ist = st.view(torch.int32)
        ist[fn.GS_TRACKER] = int(sd["growth_tracker"])
        ist[fn.GS_SKIPPED] = int(sd["skipped_steps"])
        self.state.copy_(st)  # in place: a captured graph keeps the tensor
        self.growth_factor = float(sd["growth_factor"])
        self.backoff_factor = float(sd["backoff_factor"])
        self.growth_interval = int(sd["growth_interval"])
