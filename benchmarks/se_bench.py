"""Device time of the squeeze-and-excitation kernels (csrc/se.hip), resident
against streamed, and both against the SE block composed from the ops that
existed before them.

Shapes: the four ResNet-18 CIFAR block exits at batch 8192 (32x32x64,
16x16x128, 8x8x256, 4x4x512), reduction 16, bf16, residual + ReLU.

  fwd_*  forward only (grad enabled: side outputs and mask written)
  fb_*   forward + backward (dx, dres and the four parameter gradients)

  *_res / *_str   the new op forced onto the resident / streamed path
  *_auto          ops.squeeze_excite (the path rule)
  *_composed      global_avg_pool, two ops.linear, torch.sigmoid, eager
                  multiply, add and relu

A window is `iters` calls between two device events. Every round runs one
window of each arm, in turn, so the arms see the same machine; the band of
an arm is (max - min) / median over its rounds. An arm the resident path
cannot serve is reported as null.

    python benchmarks/se_bench.py [--rounds 7] [--iters 10] [--scale 1.0]
                                  [--out results.json]

--scale shrinks the batch (for a rehearsal). Needs a GPU: there is no CPU
mode. Results: profiles/r15_se.md.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import mi355x.ops as ops  # noqa: E402
from mi355x.ops import functional as fn  # noqa: E402

SHAPES = [(8192, 32, 32, 64), (8192, 16, 16, 128), (8192, 8, 8, 256),
          (8192, 4, 4, 512)]
REDUCTION = 16


def _window(f, iters):
    a, b = torch.cuda.Event(True), torch.cuda.Event(True)
    a.record()
    for _ in range(iters):
        f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def _serves(f):
    try:
        f()
    except RuntimeError as e:
        if "resident path" in str(e):
            return False
        raise
    return True


def bench_shape(N, H, W, C, rounds, iters):
    dev, bf = "cuda", torch.bfloat16
    Cr = C // REDUCTION
    x = torch.randn(N, H, W, C, device=dev, dtype=bf).requires_grad_()
    res = torch.randn(N, H, W, C, device=dev, dtype=bf).requires_grad_()
    dy = torch.randn(N, H, W, C, device=dev, dtype=bf)
    w1 = (torch.randn(Cr, C, device=dev) / C ** 0.5).requires_grad_()
    b1 = torch.zeros(Cr, device=dev).requires_grad_()
    w2 = (torch.randn(C, Cr, device=dev) / Cr ** 0.5).requires_grad_()
    b2 = torch.zeros(C, device=dev).requires_grad_()
    leaves = (x, w1, b1, w2, b2, res)

    def fused(path):
        if path is None:
            return lambda: ops.squeeze_excite(x, w1, b1, w2, b2, res, "relu")
        return lambda: fn._SEFn.apply(x, w1, b1, w2, b2, res, 1, True, path,
                                      0)

    def composed():
        s = ops.global_avg_pool(x)
        z = ops.linear(s, w1, b1, "relu")
        g = torch.sigmoid(ops.linear(z, w2, b2))
        return torch.relu(x * g[:, None, None, :] + res)

    def with_backward(f):
        return lambda: torch.autograd.grad(f(), leaves, dy)

    fwd = {"res": fused(1), "str": fused(2), "auto": fused(None),
           "composed": composed}
    arms = {f"fwd_{k}": f for k, f in fwd.items()}
    arms.update({f"fb_{k}": with_backward(f) for k, f in fwd.items()})
    live = {k: f for k, f in arms.items() if _serves(f)}
    for f in live.values():
        _window(f, 3)
    ms = {k: [] for k in live}
    for _ in range(rounds):
        for k, f in live.items():
            ms[k].append(_window(f, iters))
    out = {"shape": [N, H, W, C], "Cr": Cr,
           "tensor_MiB": x.numel() * 2 / 2 ** 20}
    for k in arms:
        if k not in live:
            out[k] = None
            continue
        med = statistics.median(ms[k])
        out[k] = {"median_ms": round(med, 4), "min_ms": round(min(ms[k]), 4),
                  "max_ms": round(max(ms[k]), 4),
                  "band": round((max(ms[k]) - min(ms[k])) / med, 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("se_bench: needs a GPU")
    results = []
    for N, H, W, C in SHAPES:
        r = bench_shape(max(1, int(N * args.scale)), H, W, C, args.rounds,
                        args.iters)
        print(json.dumps(r), flush=True)
        results.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
