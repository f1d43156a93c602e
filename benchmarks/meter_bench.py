"""What metrics.DeviceMeter costs and what it saves, on one GPU.

Part "update": one metering update on bf16 logits, at B=8192/C=10 (the
CIFAR evaluation batch) and B=2048/C=1000.

  a  DeviceMeter.update (loss, top-1, top-5)        2 launches
  b  what the scripts run per batch today, without
     their .item(): torch.max, ==, sum              4 launches (top-1 only;
                                                    torch.max is a reduce
                                                    and a copy)
  c  (b)'s torch.max, then DistAccuracy.update      6 launches (max x2, ==,
                                                    sum, stack, add) and one
                                                    H2D copy of a host-built
                                                    tensor
  d  (a) with one wave per row (pack = 64) where (a) packs four rows per
     wave (C <= 16): the row-packing A/B

The launch counts are those of a kernel trace of this part (rocprofv3
--kernel-trace --stats), which also gives the kernels' own device times. The
timed windows here are `steps` back-to-back updates between two device
synchronisations on the host clock, so they hold launch cost as well.

Part "loop": the serial training loop on synthetic data, Net at batch 2048
and ResNet-18 at batch 8192, bf16, the same seeded inputs:

  a  loss.item() after every step, as the scripts do by default
  b  meter.update(outputs, labels, loss=loss.detach()) after every step and
     one meter.compute() at the end of the window (MI355X_DEVICE_METER=1)

and, apart from the timing, 20 steps of either loop from the same seed: the
final parameters must be bit-identical (the meter must not change training).

Windows alternate a, b, (c, d,) a within every round, so each round holds two
windows of arm (a): all (a) windows together give the noise band that a
difference between arms has to be read against.

    python benchmarks/meter_bench.py [--part update,loop] [--rounds 6]
                                     [--shapes 8192x10,2048x1000]
                                     [--out results.json]

Prints one JSON line per case. Needs a GPU: there is no CPU mode. Results:
profiles/r12_meter.md.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lars_bench import N_POOL, _interleave  # noqa: E402
from mi355x import amp, optim  # noqa: E402
from mi355x.metrics import DeviceMeter, DistAccuracy  # noqa: E402
from mi355x.models import build_model  # noqa: E402
from mi355x.ops import cross_entropy, ext  # noqa: E402
from mi355x.parallel.flat import FlatState  # noqa: E402

UPDATE_SHAPES = [(8192, 10), (2048, 1000)]
LOOP_CASES = [("net", 2048), ("resnet18", 8192)]
LAUNCHES = {"a": 2, "b": 4, "c": "6 + one H2D copy", "d": 2}


def run_update(B, C, steps, warmup, rounds, device):
    g = torch.Generator().manual_seed(B + C)
    logits = (torch.randn(B, C, generator=g) * 3).to(torch.bfloat16).to(device)
    y = torch.randint(0, C, (B,), generator=g).to(device)
    meter = DeviceMeter(C, topk=5, device=device)
    wave = DeviceMeter(C, topk=5, device=device)
    acc = DistAccuracy(device=device)

    def torch_ops(i):
        _, pred = torch.max(logits, 1)
        return (pred == y).sum()

    def dist_accuracy(i):
        _, pred = torch.max(logits, 1)
        acc.update(pred, y)

    def one_wave_per_row(i):
        ext().meter_update(wave.state, wave.slab, logits, y, None, None, 5,
                           None, None, 64)

    arms = {"a": lambda i: meter.update(logits, y), "b": torch_ops,
            "c": dist_accuracy}
    if C <= 16:
        arms["d"] = one_wave_per_row
    res, ms = _interleave(arms, steps, warmup, rounds)
    med = {k: statistics.median(ms[k]) for k in arms if k != "a"}
    med["a"] = res["a_median_all"]
    r = meter.compute()
    res.update({
        "part": "update", "B": B, "C": C, "dtype": "bf16",
        "launches_per_update": {k: LAUNCHES[k] for k in arms},
        "median_us": {k: round(v * 1e3, 2) for k, v in sorted(med.items())},
        "a_band_us": round(res["a_band"] * 1e3, 2),
        "meter_over_torch_ops": round(med["a"] / med["b"], 4),
        "meter_over_dist_accuracy": round(med["a"] / med["c"], 4),
        # the arms agree on what they count
        "top1": {"meter": r["top1"],
                 "torch_ops": torch_ops(0).item() / B,
                 "dist_accuracy": acc.compute()},
    })
    if "d" in arms:
        res["packed_over_one_wave_per_row"] = round(med["a"] / med["d"], 4)
        res["top1"]["one_wave_per_row"] = wave.compute()["top1"]
    return res


class LoopArm:
    """A model + SGD on pool batches; step(i) is one iteration of the
    scripts' training loop, logging with loss.item() or with the meter."""

    def __init__(self, model, metered, pool_x, pool_y, device, window=None):
        self.pool_x, self.pool_y = pool_x, pool_y
        torch.manual_seed(1234)
        self.net = build_model(model, num_classes=10).to(device)
        self.flat = FlatState(self.net)
        self.opt = optim.SGD(self.flat, lr=0.01, momentum=0.9)
        self.meter = DeviceMeter(10, device=device) if metered else None
        self.window = window  # (first timed step, steps per window)
        self.running = 0.0
        self.read = None

    def step(self, i):
        x, y = self.pool_x[i % N_POOL], self.pool_y[i % N_POOL]
        self.opt.zero_grad()
        out = self.net(x)
        loss = cross_entropy(out, y)
        loss.backward()
        self.opt.step()
        if self.meter is None:
            self.running += loss.item()
            return
        self.meter.update(out, y, loss=loss.detach())
        if self.window is not None:
            first, per = self.window
            if i >= first and (i - first + 1) % per == 0:
                self.read = self.meter.compute(sync=False)
                self.meter.reset()


def run_loop(model, batch, steps, warmup, rounds, device):
    g = torch.Generator(device="cpu").manual_seed(4321)
    pool_x = [torch.randn(batch, 3, 32, 32, generator=g).to(device)
              for _ in range(N_POOL)]
    pool_y = [torch.randint(0, 10, (batch,), generator=g).to(device)
              for _ in range(N_POOL)]
    arms = {"a": LoopArm(model, False, pool_x, pool_y, device),
            "b": LoopArm(model, True, pool_x, pool_y, device,
                         window=(warmup, steps))}
    res, ms = _interleave({k: a.step for k, a in arms.items()}, steps,
                          warmup, rounds)
    a_med, b_med = res["a_median_all"], statistics.median(ms["b"])
    # the meter must not change the training: the same 20 steps either way
    twins = [LoopArm(model, metered, pool_x, pool_y, device)
             for metered in (False, True)]
    for arm in twins:
        for i in range(20):
            arm.step(i)
    torch.cuda.synchronize()
    res.update({
        "part": "loop", "model": model, "batch": batch, "dtype": "bf16",
        "images_per_s": {"item_every_step": round(batch / a_med * 1e3, 1),
                         "meter": round(batch / b_med * 1e3, 1)},
        "b_minus_a_ms": round(b_med - a_med, 4),
        "speedup": round(a_med / b_med, 4),
        "outside_a_band": bool(abs(b_med - a_med) > res["a_band"]),
        "last_window_loss": arms["b"].read["loss"],
        "params_bit_identical": bool(torch.equal(twins[0].flat.flat_param,
                                                 twins[1].flat.flat_param)),
        "twin_mean_loss": {"item": twins[0].running / 20,
                           "meter": twins[1].meter.compute()["loss"]},
    })
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="update,loop")
    ap.add_argument("--shapes", default=",".join(
        f"{b}x{c}" for b, c in UPDATE_SHAPES), help="BxC of the update part")
    ap.add_argument("--update-steps", type=int, default=2000,
                    help="updates per timed window")
    ap.add_argument("--steps", type=int, default=0,
                    help="train steps per timed window (0: 200 for net, 10 "
                         "for resnet18)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default=None, help="also write the lines here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("meter_bench.py measures on a GPU; none found")
    device = torch.device("cuda", 0)
    amp.set_compute_dtype(torch.bfloat16)
    lines = []
    parts = args.part.split(",")
    if "update" in parts:
        for B, C in (map(int, s.split("x")) for s in args.shapes.split(",")):
            lines.append(json.dumps(run_update(
                B, C, args.update_steps, max(args.warmup, 50), args.rounds,
                device)))
            print(lines[-1], flush=True)
    if "loop" in parts:
        for model, batch in LOOP_CASES:
            steps = args.steps or (200 if model == "net" else 10)
            lines.append(json.dumps(run_loop(model, batch, steps, args.warmup,
                                             args.rounds, device)))
            print(lines[-1], flush=True)
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
