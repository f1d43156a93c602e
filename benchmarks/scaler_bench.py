"""A/B of fp16 dynamic loss scaling: host GradScaler vs DeviceGradScaler.

fp16 ResNet-18, synthetic 32x32 data, one GPU, one process. Per batch size
three arms train their own (identically seeded) copy of the model:

  a  amp.GradScaler, eager       isfinite().all().item() + host branch
  b  amp.DeviceGradScaler, eager grad_stats + guarded SGD + scale update
  c  amp.DeviceGradScaler inside one captured graph of the whole step

Timed windows alternate a, b, c, a within every round, so each round holds
two windows of arm (a): all (a) windows together give the noise band that
a difference between arms has to be read against. A window is `steps`
steps between two device synchronisations, timed with the host clock.

    python benchmarks/scaler_bench.py [--batches 256,8192] [--rounds 6]
                                      [--out results.json]

Prints one JSON line per batch size: per-arm median/min/max ms per step,
the (a) band (range of all its windows), the per-round paired differences
(b and c against the mean of the two (a) windows around them, next to the
mean |a1 - a2|), and whether (b) is within the (a) noise by either
measure. Needs a GPU: there is no CPU mode. Results:
profiles/r07_device_scaler.md.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mi355x import amp, optim  # noqa: E402
from mi355x.models import build_model  # noqa: E402
from mi355x.ops import cross_entropy  # noqa: E402
from mi355x.parallel.flat import FlatState  # noqa: E402

INIT_SCALE = 2.0 ** 14
GROWTH_INTERVAL = 200  # bench.py's fp16 setting
N_POOL = 2


class Arm:
    """One model + optimizer + scaler; step(i) trains on pool batch i."""

    def __init__(self, kind, pool_x, pool_y, device):
        self.kind = kind
        self.pool_x, self.pool_y = pool_x, pool_y
        torch.manual_seed(1234)
        self.net = build_model("resnet18", num_classes=10).to(device)
        self.flat = FlatState(self.net)
        self.opt = optim.SGD(self.flat, lr=0.1, momentum=0.9)
        if kind == "a":
            self.scaler = amp.GradScaler(init_scale=INIT_SCALE,
                                         growth_interval=GROWTH_INTERVAL)
            self.skipped = 0
        else:
            self.scaler = amp.DeviceGradScaler(
                init_scale=INIT_SCALE, growth_interval=GROWTH_INTERVAL,
                device=device)
        self.loss = None
        if kind == "c":
            self._capture()

    def _train(self, x, y):
        self.opt.zero_grad()
        loss = cross_entropy(self.net(x), y)
        if self.kind == "a":
            used = self.scaler.scale_value
            (loss * used).backward()
            if self.scaler.step_ok(self.flat.flat_grad):
                self.opt.grad_scale = 1.0 / used
                self.opt.step()
            else:
                self.skipped += 1
        else:
            self.scaler.scale(loss).backward()
            self.opt.step(scaler=self.scaler)
        return loss

    def _capture(self):
        self.static_x = self.pool_x[0].clone()
        self.static_y = self.pool_y[0].clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):
                self._train(self.static_x, self.static_y)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.static_loss = self._train(self.static_x, self.static_y)

    def step(self, i):
        x, y = self.pool_x[i % N_POOL], self.pool_y[i % N_POOL]
        if self.kind == "c":
            self.static_x.copy_(x)
            self.static_y.copy_(y)
            self.graph.replay()
            self.loss = self.static_loss
        else:
            self.loss = self._train(x, y)

    def window(self, steps, start):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(start, start + steps):
            self.step(i)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    def summary(self):
        skipped = (self.skipped if self.kind == "a"
                   else self.scaler.skipped_steps)
        return {"final_scale": self.scaler.scale_value, "skipped": skipped,
                "loss": round(float(self.loss.item()), 4)}


def _stats(ms):
    return {"median": round(statistics.median(ms), 3),
            "min": round(min(ms), 3), "max": round(max(ms), 3),
            "windows": [round(v, 3) for v in ms]}


def run_batch(batch, steps, warmup, rounds, device):
    g = torch.Generator(device="cpu").manual_seed(4321)
    pool_x = [torch.randn(batch, 3, 32, 32, generator=g).to(device)
              for _ in range(N_POOL)]
    pool_y = [torch.randint(0, 10, (batch,), generator=g).to(device)
              for _ in range(N_POOL)]
    arms = {k: Arm(k, pool_x, pool_y, device) for k in "abc"}
    for arm in arms.values():
        arm.window(warmup, 0)
    ms = {"a1": [], "b": [], "c": [], "a2": []}
    pos = warmup
    for _ in range(rounds):
        for slot in ("a1", "b", "c", "a2"):
            ms[slot].append(arms[slot[0]].window(steps, pos))
        pos += steps
    a_all = ms["a1"] + ms["a2"]
    band = max(a_all) - min(a_all)
    a_med = statistics.median(a_all)
    b_med = statistics.median(ms["b"])
    # paired by round: a1 and a2 bracket b and c, so their mean cancels a
    # drift that is linear over the round (clocks settling, a busy host)
    a_mid = [(p + q) / 2 for p, q in zip(ms["a1"], ms["a2"])]
    a_gap = statistics.mean(abs(p - q) for p, q in zip(ms["a1"], ms["a2"]))
    b_pair = statistics.mean(b - a for b, a in zip(ms["b"], a_mid))
    c_pair = statistics.mean(c - a for c, a in zip(ms["c"], a_mid))
    return {
        "paired": {"a1_vs_a2_mean_abs": round(a_gap, 3),
                   "b_minus_a_mean": round(b_pair, 3),
                   "c_minus_a_mean": round(c_pair, 3),
                   "b_within_a1_vs_a2": bool(b_pair <= a_gap)},
        "batch": batch, "steps_per_window": steps, "rounds": rounds,
        "ms_per_step": {k: _stats(v) for k, v in ms.items()},
        "a_median_all": round(a_med, 3),
        # noise: the range of all windows of arm (a), and how far its two
        # slots' medians lie apart
        "a_band": round(band, 3),
        "a1_vs_a2_medians": round(abs(statistics.median(ms["a1"])
                                      - statistics.median(ms["a2"])), 3),
        "b_minus_a": round(b_med - a_med, 3),
        "c_minus_a": round(statistics.median(ms["c"]) - a_med, 3),
        "b_within_a_band": bool(b_med - a_med <= band),
        "arms": {k: arm.summary() for k, arm in arms.items()},
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,8192")
    ap.add_argument("--steps", type=int, default=None,
                    help="steps per timed window (default: 10 at batch >= "
                         "2048, 60 below: about a second either way)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default=None, help="also write the lines here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scaler_bench.py measures on a GPU; none found")
    device = torch.device("cuda", 0)
    amp.set_compute_dtype(torch.float16)
    lines = []
    for batch in (int(b) for b in args.batches.split(",")):
        steps = args.steps or (10 if batch >= 2048 else 60)
        res = run_batch(batch, steps, args.warmup, args.rounds, device)
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
