"""What optim.LARS costs against the SGD steps, on one GPU.

Part "opt": the optimizer step alone on the flat buffers of ResNet-18 and
ResNet-50 (the models' real tensor offsets; random weights and gradients).

  a  ops.sgd_step                                   one kernel
  b  guarded SGD: grad_stats + sgd_step_guarded + scaler_update
  c  LARS: lars_stats + lars_step + scaler_update

(b) and (c) run through optim.SGD / optim.LARS with a max_grad_norm no
gradient reaches, so both carry the same guard. By memory traffic (b) moves
6 buffer-sized streams (g; w, g, m in; w, m out) and (c) 7 (w and g; then
the same six): the expected ratio c/b is 7/6.

Part "step": the whole eager ResNet-18 bf16 train step at batch 8192,
guarded SGD (a) against LARS (b).

Timed windows alternate a, b, (c,) a within every round, so each round
holds two windows of arm (a): all (a) windows together give the noise band
that a difference between arms has to be read against. A window is `steps`
steps between two device synchronisations, timed with the host clock.

    python benchmarks/lars_bench.py [--part opt,step] [--rounds 6]
                                    [--out results.json]

Prints one JSON line per model (opt) and one for the train step. Needs a
GPU: there is no CPU mode. For per-kernel times run the opt part alone
under a kernel trace. Results: profiles/r09_lars.md.
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

NEVER_CLIPS = 1e30
N_POOL = 2


def _window(fn, steps, start=0):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(start, start + steps):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def _stats(ms):
    return {"median": round(statistics.median(ms), 4),
            "min": round(min(ms), 4), "max": round(max(ms), 4),
            "windows": [round(v, 4) for v in ms]}


def _interleave(arms, steps, warmup, rounds):
    """arms: {"a": fn, "b": fn, ...}; -> per-slot window lists and the
    noise figures of arm (a)."""
    for fn in arms.values():
        _window(fn, warmup)
    slots = ["a1"] + [k for k in arms if k != "a"] + ["a2"]
    ms = {s: [] for s in slots}
    pos = warmup
    for _ in range(rounds):
        for s in slots:
            ms[s].append(_window(arms[s[0]], steps, pos))
        pos += steps
    a_all = ms["a1"] + ms["a2"]
    # paired by round: a1 and a2 bracket the other arms, so their mean
    # cancels a drift that is linear over the round
    a_mid = [(p + q) / 2 for p, q in zip(ms["a1"], ms["a2"])]
    res = {
        "steps_per_window": steps, "rounds": rounds,
        "ms_per_step": {k: _stats(v) for k, v in ms.items()},
        "a_median_all": round(statistics.median(a_all), 4),
        "a_band": round(max(a_all) - min(a_all), 4),
        "a1_vs_a2_mean_abs": round(statistics.mean(
            abs(p - q) for p, q in zip(ms["a1"], ms["a2"])), 4),
    }
    for k in slots[1:-1]:
        res[f"{k}_minus_a_paired_mean"] = round(statistics.mean(
            v - a for v, a in zip(ms[k], a_mid)), 4)
    return res, ms


def run_opt(model, steps, warmup, rounds, device):
    torch.manual_seed(1234)
    arms, flats, opts = {}, {}, {}
    for kind in "abc":
        net = build_model(model, num_classes=10).to(device)
        flat = FlatState(net)
        flat.flat_grad.normal_(std=1e-2)
        if kind == "a":
            opt = optim.SGD(flat, lr=1e-4, momentum=0.9, weight_decay=5e-4)
        elif kind == "b":
            opt = optim.SGD(flat, lr=1e-4, momentum=0.9, weight_decay=5e-4,
                            max_grad_norm=NEVER_CLIPS)
        else:
            opt = optim.LARS(flat, lr=1e-4, momentum=0.9, weight_decay=5e-4,
                             max_grad_norm=NEVER_CLIPS)
        flats[kind], opts[kind] = flat, opt
        arms[kind] = (lambda i, o=opt: o.step())
    res, ms = _interleave(arms, steps, warmup, rounds)
    flat = flats["c"]
    med = {k: statistics.median(ms[k]) for k in ("b", "c")}
    nbytes = flat.numel * 4
    res.update({
        "part": "opt", "model": model, "numel": flat.numel,
        "tensors": len(flat.params),
        "misaligned_starts": sum(1 for p in flat.params
                                 if flat.offsets[id(p)][0] % 4),
        "lars_over_guarded_sgd": round(med["c"] / med["b"], 4),
        "expected_by_traffic": round(7 / 6, 4),
        "guarded_sgd_gbytes_per_s": round(6 * nbytes / med["b"] / 1e6, 1),
        "lars_gbytes_per_s": round(7 * nbytes / med["c"] / 1e6, 1),
        "skipped": {k: opts[k].skipped_steps for k in "bc"},
        "finite": bool(torch.isfinite(flat.flat_param).all()),
    })
    return res


class TrainArm:
    """ResNet-18 + optimizer; step(i) trains on pool batch i."""

    def __init__(self, kind, pool_x, pool_y, device, lr):
        self.pool_x, self.pool_y = pool_x, pool_y
        torch.manual_seed(1234)
        self.net = build_model("resnet18", num_classes=10).to(device)
        self.flat = FlatState(self.net)
        cls = optim.SGD if kind == "a" else optim.LARS
        self.opt = cls(self.flat, lr=lr, momentum=0.9, weight_decay=5e-4,
                       max_grad_norm=NEVER_CLIPS)
        self.loss = None

    def step(self, i):
        x, y = self.pool_x[i % N_POOL], self.pool_y[i % N_POOL]
        self.opt.zero_grad()
        self.loss = cross_entropy(self.net(x), y)
        self.loss.backward()
        self.opt.step()


def run_step(batch, steps, warmup, rounds, device, lr):
    g = torch.Generator(device="cpu").manual_seed(4321)
    pool_x = [torch.randn(batch, 3, 32, 32, generator=g).to(device)
              for _ in range(N_POOL)]
    pool_y = [torch.randint(0, 10, (batch,), generator=g).to(device)
              for _ in range(N_POOL)]
    arms = {k: TrainArm(k, pool_x, pool_y, device, lr) for k in "ab"}
    res, ms = _interleave({k: a.step for k, a in arms.items()}, steps,
                          warmup, rounds)
    b_med = statistics.median(ms["b"])
    res.update({
        "part": "step", "model": "resnet18", "batch": batch, "lr": lr,
        "b_minus_a": round(b_med - res["a_median_all"], 4),
        "b_within_a_band": bool(abs(b_med - res["a_median_all"])
                                <= res["a_band"]),
        "loss": {k: round(float(a.loss.item()), 4) for k, a in arms.items()},
        "skipped": {k: a.opt.skipped_steps for k, a in arms.items()},
    })
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="opt,step")
    ap.add_argument("--models", default="resnet18,resnet50")
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--opt-steps", type=int, default=2000,
                    help="optimizer steps per timed window")
    ap.add_argument("--steps", type=int, default=10,
                    help="train steps per timed window")
    ap.add_argument("--lr", type=float, default=0.1,
                    help="train-step part; 0 keeps both arms on the same "
                         "weights, so their kernels see the same data")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default=None, help="also write the lines here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lars_bench.py measures on a GPU; none found")
    device = torch.device("cuda", 0)
    amp.set_compute_dtype(torch.bfloat16)
    lines = []
    parts = args.part.split(",")
    if "opt" in parts:
        for model in args.models.split(","):
            lines.append(json.dumps(run_opt(
                model, args.opt_steps, max(args.warmup, 50), args.rounds,
                device)))
            print(lines[-1], flush=True)
            torch.cuda.empty_cache()
    if "step" in parts:
        lines.append(json.dumps(run_step(args.batch, args.steps, args.warmup,
                                         args.rounds, device, args.lr)))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
