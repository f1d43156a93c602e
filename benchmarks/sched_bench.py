"""What a device-side learning-rate schedule and a fused weight EMA cost in
the optimizer step, on one GPU.

The optimizer step alone on the flat buffers of ResNet-18 and ResNet-50 (the
models' real tensor offsets; random weights and gradients), for optim.SGD
and for optim.LARS, every arm guarded with a max_grad_norm no gradient
reaches:

  a  the guarded step with a float lr              4 launches per step
  b  (a) + LRSchedule: lr read from the step clock,
     clock_advance after scaler_update             5
  c  (b) + optim.EMA fused into the update kernel  5
  d  what one would write without either: a 0-d tensor lr filled from the
     host every step (lr.fill_), the guarded step, then
     flat_ema.lerp_(flat_param, 1 - decay)         6

The launch counts are read off the code (stats: 2, update, scaler_update,
then clock_advance or fill_ and lerp_), not measured. By memory traffic the
update itself moves 5 floats per element in (a) and (b) (w, g, m read; w, m
written), 7 in (c) (e read and written as well) and 8 in (d) (lerp_ reads w
and e and writes e), which also has one more launch. The stats pass in front
reads g (SGD) or w and g (LARS) in every arm: 6, 6, 8, 9 buffer-sized
streams per step for SGD and 7, 7, 9, 10 for LARS, as lars_bench.py counts.

Timed windows alternate a, b, c, d, a within every round, so each round
holds two windows of arm (a): all (a) windows together give the noise band
that a difference between arms has to be read against. A window is `steps`
steps between two device synchronisations, timed with the host clock.

    python benchmarks/sched_bench.py [--models resnet18,resnet50]
                                     [--optims sgd,lars] [--rounds 6]
                                     [--out results.json]

Prints one JSON line per optimizer and model. Needs a GPU: there is no CPU
mode. Results: profiles/r11_sched_ema.md.
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

from lars_bench import NEVER_CLIPS, _interleave  # noqa: E402
from mi355x import amp, optim  # noqa: E402
from mi355x.models import build_model  # noqa: E402
from mi355x.parallel.flat import FlatState  # noqa: E402

DECAY = 0.999
BASE_LR = 1e-4
LAUNCHES = {"a": 4, "b": 5, "c": 5, "d": 6}
# buffer-sized streams per step: the stats pass (g, and w for LARS), the
# update's three reads and two writes, then the EMA's
STREAMS = {"sgd": {"a": 6, "b": 6, "c": 8, "d": 9},
           "lars": {"a": 7, "b": 7, "c": 9, "d": 10}}


def _schedule(total):
    return optim.LRSchedule.warmup_cosine(BASE_LR, total // 20, total)


def _arm(kind, optimizer, model, device, total):
    """-> (flat, opt, step(i))"""
    cls = optim.SGD if optimizer == "sgd" else optim.LARS
    net = build_model(model, num_classes=10).to(device)
    flat = FlatState(net)
    flat.flat_grad.normal_(std=1e-2)
    kw = dict(momentum=0.9, weight_decay=5e-4, max_grad_norm=NEVER_CLIPS)
    if kind == "a":
        opt = cls(flat, lr=BASE_LR, **kw)
        return flat, opt, (lambda i: opt.step())
    if kind == "b":
        opt = cls(flat, lr=_schedule(total), **kw)
        return flat, opt, (lambda i: opt.step())
    if kind == "c":
        opt = cls(flat, lr=_schedule(total), ema=optim.EMA(DECAY), **kw)
        return flat, opt, (lambda i: opt.step())
    lr = torch.tensor(BASE_LR, device=device)
    opt = cls(flat, lr=lr, **kw)
    host_table = _schedule(total).values.tolist()
    flat_ema = flat.flat_param.clone()
    omd = 1.0 - DECAY

    def step(i):
        lr.fill_(host_table[min(i, len(host_table) - 1)])
        opt.step()
        flat_ema.lerp_(flat.flat_param, omd)

    return flat, opt, step


def run(optimizer, model, steps, warmup, rounds, device):
    torch.manual_seed(1234)
    total = warmup + steps * rounds
    flats, opts, arms = {}, {}, {}
    for kind in "abcd":
        flats[kind], opts[kind], arms[kind] = _arm(kind, optimizer, model,
                                                   device, total)
    res, ms = _interleave(arms, steps, warmup, rounds)
    med = {k: statistics.median(ms[k]) for k in "bcd"}
    med["a"] = res["a_median_all"]
    flat = flats["c"]
    nbytes = flat.numel * 4
    c_minus_d = [c - d for c, d in zip(ms["c"], ms["d"])]
    res.update({
        "optimizer": optimizer, "model": model, "numel": flat.numel,
        "launches_per_step": LAUNCHES,
        "streams_per_step": STREAMS[optimizer],
        "median_ms": {k: round(v, 4) for k, v in sorted(med.items())},
        "gbytes_per_s": {k: round(STREAMS[optimizer][k] * nbytes / med[k]
                                  / 1e6, 1) for k in "abcd"},
        "b_over_a": round(med["b"] / med["a"], 4),
        "c_over_a": round(med["c"] / med["a"], 4),
        "d_over_a": round(med["d"] / med["a"], 4),
        "c_over_d": round(med["c"] / med["d"], 4),
        "c_minus_d_paired_mean": round(statistics.mean(c_minus_d), 4),
        "c_minus_d_paired_max": round(max(c_minus_d), 4),
        # the requirement: fused no slower than separate, beyond the spread
        "c_not_slower_than_d": bool(med["c"] <= med["d"] + res["a_band"]),
        "clock_step": {k: opts[k].clock_step for k in "bc"},
        "skipped": {k: opts[k].skipped_steps for k in "abcd"},
        "finite": bool(torch.isfinite(flat.flat_param).all()
                       and torch.isfinite(opts["c"].ema.flat_ema).all()),
    })
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="resnet18,resnet50")
    ap.add_argument("--optims", default="sgd,lars")
    ap.add_argument("--steps", type=int, default=2000,
                    help="optimizer steps per timed window")
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default=None, help="also write the lines here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sched_bench.py measures on a GPU; none found")
    device = torch.device("cuda", 0)
    amp.set_compute_dtype(torch.bfloat16)
    lines = []
    for optimizer in args.optims.split(","):
        for model in args.models.split(","):
            lines.append(json.dumps(run(optimizer, model, args.steps,
                                        args.warmup, args.rounds, device)))
            print(lines[-1], flush=True)
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
