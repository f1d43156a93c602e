"""What optim.AdamW and optim.LAMB cost, on one GPU: the optimizer step alone
on the flat buffers of ResNet-18 and ResNet-50 (the models' real tensor
offsets; random weights and gradients), once plain and once with an
LRSchedule and an EMA.

  a  guarded SGD: grad_stats + sgd_step_guarded + scaler_update
  b  LARS: lars_stats + lars_step + scaler_update
  c  AdamW: grad_stats + adam_step + scaler_update + clock_advance
  d  LAMB: grad_stats + lamb_step (3 kernels) + scaler_update + clock_advance
  e  torch.optim.AdamW on the same parameters (fused=True, else foreach),
     with a separate flat_ema.lerp_ in the EMA configuration

All of ours carry the same guard (a max_grad_norm no gradient reaches). By
memory traffic per element (a) moves 6 floats, (b) 7, (c) 8, (d) 11: the
expected ratios to (a) are 7/6, 8/6 and 11/6 (plus 2 floats each with an EMA).
(e) has no guard: no norm, no skip decision, host-side step counter.

Windows alternate a, b, c, d, e, a within every round (lars_bench's
scheme): the two (a) windows of all rounds give the run-to-run band that a
difference between arms has to be read against. Launches per step are
counted from one profiled step of each arm.

    python benchmarks/adam_bench.py [--models resnet18,resnet50]
                                    [--rounds 6] [--out results.json]

Prints one JSON line per model and configuration. Needs a GPU. Results:
profiles/r16_adam.md.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from lars_bench import NEVER_CLIPS, _interleave  # noqa: E402
from mi355x import optim  # noqa: E402
from mi355x.models import build_model  # noqa: E402
from mi355x.parallel.flat import FlatState  # noqa: E402

TRAFFIC = {"a": 6, "b": 7, "c": 8, "d": 11}  # floats per element, no EMA
NAMES = {"a": "guarded_sgd", "b": "lars", "c": "adamw", "d": "lamb",
         "e": "torch_adamw"}


def _torch_adamw(flat, ema):
    kw = dict(lr=1e-4, weight_decay=1e-2)
    try:
        opt = torch.optim.AdamW(flat.params, fused=True, **kw)
        form = "fused"
    except (RuntimeError, TypeError):
        opt = torch.optim.AdamW(flat.params, foreach=True, **kw)
        form = "foreach"
    if not ema:
        return opt.step, form
    e = flat.flat_param.clone()

    def step():
        opt.step()
        e.lerp_(flat.flat_param, 1e-3)
    return step, form


def _launches(step):
    """GPU kernels launched by one step, from a profiled call."""
    from torch.profiler import ProfilerActivity, profile
    step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    return sum(1 for ev in prof.events()
               if ev.device_type == torch.autograd.DeviceType.CUDA)


def run(model, clocked, steps, warmup, rounds, device):
    torch.manual_seed(1234)
    arms, steps_of, form, flat = {}, {}, None, None
    for kind in "abcde":
        flat = FlatState(build_model(model, num_classes=10).to(device))
        flat.flat_grad.normal_(std=1e-2)
        kw = dict(max_grad_norm=NEVER_CLIPS)
        if clocked and kind != "e":
            kw["ema"] = optim.EMA(0.999)
        lr = optim.LRSchedule.warmup_cosine(1e-4, 100, 10 ** 6) if clocked \
            else 1e-4
        if kind == "a":
            step = optim.SGD(flat, lr, momentum=0.9, weight_decay=5e-4,
                             **kw).step
        elif kind == "b":
            step = optim.LARS(flat, lr, momentum=0.9, weight_decay=5e-4,
                              **kw).step
        elif kind == "c":
            step = optim.AdamW(flat, lr, **kw).step
        elif kind == "d":
            step = optim.LAMB(flat, lr, **kw).step
        else:
            step, form = _torch_adamw(flat, clocked)
        steps_of[kind] = step
        arms[kind] = (lambda i, s=step: s())
    res, ms = _interleave(arms, steps, warmup, rounds)
    a = res["a_median_all"]
    med = {k: statistics.median(ms[k]) for k in "bcde"}
    res.update({
        "model": model, "schedule_and_ema": clocked, "numel": flat.numel,
        "tensors": len(flat.params), "torch_adamw_form": form,
        "median_ms": {NAMES[k]: round(v, 4) for k, v in med.items()},
        "over_guarded_sgd": {NAMES[k]: round(v / a, 4)
                             for k, v in med.items()},
        "expected_by_traffic": {
            NAMES[k]: round((TRAFFIC[k] + 2 * clocked) /
                            (TRAFFIC["a"] + 2 * clocked), 4) for k in "bcd"},
        "adamw_over_torch_adamw": round(med["c"] / med["e"], 4),
        "a_band_over_median": round(res["a_band"] / a, 4),
    })
    try:
        res["launches"] = {NAMES[k]: _launches(s)
                           for k, s in steps_of.items()}
    except Exception as err:  # the timings above stand without the count
        res["launches"] = None
        res["launches_error"] = repr(err)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="resnet18,resnet50")
    ap.add_argument("--opt-steps", type=int, default=1000,
                    help="optimizer steps per timed window")
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default=None, help="also write the lines here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adam_bench.py measures on a GPU; none found")
    device = torch.device("cuda", 0)
    lines = []
    for model in args.models.split(","):
        for clocked in (False, True):
            lines.append(json.dumps(run(model, clocked, args.opt_steps,
                                        args.warmup, args.rounds, device)))
            print(lines[-1], flush=True)
            if args.out:
                with open(args.out, "w") as f:
                    f.write("\n".join(lines) + "\n")
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
