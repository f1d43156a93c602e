"""Distributed metrics (SURVEY.md N14 — torchmetrics is not installed).

DistAccuracy mirrors the reference's
torchmetrics.Accuracy(dist_sync_on_step=True) usage
(/root/reference/cifar_example_ddp.py:124-136): accumulates
(correct, total) and all-reduces the two int64 counters across ranks —
either on every update (dist_sync_on_step) or once at compute().

DeviceMeter keeps loss, top-1/top-k counts and a confusion matrix on the
device (kernels: mi355x/csrc/meter.hip) and is read back, and reduced over
the ranks, only when compute() is called.
"""

from __future__ import annotations

import torch
import torch.distributed as dist


class DistAccuracy:
    def __init__(self, dist_sync_on_step: bool = False, device=None):
        self.dist_sync_on_step = dist_sync_on_step
        self.device = device or torch.device("cpu")
        self.reset()

    def reset(self):
        self.state = torch.zeros(2, dtype=torch.long, device=self.device)

    def _sync(self, t):
        if dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(t)
        return t

    def update(self, preds: torch.Tensor, target: torch.Tensor):
        if preds.dim() > 1:
            preds = preds.argmax(dim=-1)
        delta = torch.stack([
            (preds == target).sum().to(self.state.device),
            torch.tensor(target.numel(), device=self.state.device),
        ])
        if self.dist_sync_on_step:
            delta = self._sync(delta.clone())
        self.state += delta

    def compute(self) -> float:
        s = self.state if self.dist_sync_on_step else self._sync(self.state.clone())
        return (s[0].float() / s[1].clamp(min=1).float()).item()


class DeviceMeter:
    """Loss, top-1 / top-k accuracy and (optionally) the confusion matrix of
    a stream of batches, kept on the device: ``update`` launches two kernels
    on the current stream (capturable, no allocation, no host read),
    ``compute`` is the only call that reads back.

        meter = DeviceMeter(10, topk=5, confusion=True, device=dev)
        meter.update(logits, target)              # or loss=loss.detach()
        meter.compute()  ->  {"rows", "top1", "top5", "loss", "bad_rows",
                              "updates", "confusion", "per_class"}

    ``target`` is an int64 (B,) tensor or an ops.MixTarget (the row's label
    is then the heavier of the two, y_a at lam == 0.5). What a row counts
    for is defined in ops.meter_update. ``loss`` in the result is the mean
    nll per row (or the row-weighted mean of the losses handed to
    ``update``), and NaN as soon as one row was bad (a label outside
    [0,C) or a non-finite lse), so a divergence shows. The state layout is
    documented in mi355x/csrc/meter.hip."""

    def __init__(self, num_classes: int, topk: int = 5,
                 confusion: bool = False, device=None):
        from mi355x.ops import functional as Fn

        if num_classes < 1 or topk < 1:
            raise ValueError("DeviceMeter: num_classes and topk must be >= 1")
        self.num_classes = int(num_classes)
        self.topk = int(topk)
        self.device = torch.device(device or "cpu")
        self.state = torch.zeros(Fn.MT_LEN, dtype=torch.int64,
                                 device=self.device)
        # per-block partials of the row kernel; the CPU twin needs none
        self.slab = (torch.zeros(Fn.METER_SLAB, dtype=torch.int64,
                                 device=self.device)
                     if self.device.type == "cuda" else None)
        self.confusion = (torch.zeros(self.num_classes, self.num_classes,
                                      dtype=torch.int64, device=self.device)
                          if confusion else None)

    def reset(self):
        """Zero the meter on the device (capturable)."""
        self.state.zero_()
        if self.confusion is not None:
            self.confusion.zero_()

    def update(self, logits: torch.Tensor, target, loss=None):
        from mi355x.ops import MixTarget, meter_update

        if logits.dim() != 2 or logits.shape[1] != self.num_classes:
            raise ValueError(f"DeviceMeter: logits must be (B, "
                             f"{self.num_classes}), got {tuple(logits.shape)}")
        if isinstance(target, MixTarget):
            y_a, y_b, lam = target
        else:
            y_a, y_b, lam = target, None, None
        meter_update(self.state, self.slab, logits, y_a, y_b, lam,
                     k=self.topk, loss=loss, confusion=self.confusion)

    def merge(self, other: "DeviceMeter"):
        """Add another meter's state into this one, on the device (no host
        read): how a short logging window feeds a whole-run total."""
        from mi355x.ops import functional as Fn

        ls = slice(Fn.MT_LOSS_SUM, Fn.MT_LOSS_SUM + 1)
        total = (self.state[ls].view(torch.float64)
                 + other.state[ls].view(torch.float64))
        self.state += other.state
        self.state[ls].view(torch.float64).copy_(total)
        if self.confusion is not None and other.confusion is not None:
            self.confusion += other.confusion

    def compute(self, sync: bool = True) -> dict:
        """One device-to-host copy of the state (and the matrix). With
        ``sync`` and an initialised process group of more than one rank the
        states are summed over the ranks first, in one all-reduce of a
        float64 vector: the counts stay exact below 2^53."""
        from mi355x.ops import functional as Fn

        ls = slice(Fn.MT_LOSS_SUM, Fn.MT_LOSS_SUM + 1)
        vec = self.state.double()
        vec[ls] = self.state[ls].view(torch.float64)
        if self.confusion is not None:
            vec = torch.cat([vec, self.confusion.reshape(-1).double()])
        if sync and dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(vec)
        host = vec.cpu()
        rows, c1, ck, bad = (int(host[i]) for i in (
            Fn.MT_ROWS, Fn.MT_CORRECT1, Fn.MT_CORRECTK, Fn.MT_BAD))
        nan = float("nan")
        out = {
            "rows": rows,
            "top1": c1 / rows if rows else nan,
            f"top{self.topk}": ck / rows if rows else nan,
            "loss": (float(host[Fn.MT_LOSS_SUM]) / rows
                     if rows and bad == 0 else nan),
            "bad_rows": bad,
            "updates": int(host[Fn.MT_UPDATES]),
        }
        if self.confusion is not None:
            C = self.num_classes
            conf = host[Fn.MT_LEN:].to(torch.int64).reshape(C, C)
            seen = conf.sum(dim=1)
            out["confusion"] = conf
            out["per_class"] = torch.where(
                seen > 0, conf.diagonal().double() / seen.double(),
                torch.full((C,), nan, dtype=torch.float64))
        return out
