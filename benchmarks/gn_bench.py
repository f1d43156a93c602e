"""Device time of the GroupNorm kernels (csrc/gn.hip), resident against
streamed, and both against BatchNorm's kernels on the same tensor.

Shapes: the four ResNet-18 CIFAR activations at batch 8192 (32x32x64,
16x16x128, 8x8x256, 4x4x512) and the 112x112x64 ImageNet stem at batch 256,
G = 32, bf16, residual + ReLU (the block-exit form; BN gets the same).

  forward   gn resident | gn streamed | bn_stats + bn_finalize + bn_apply
  backward  gn resident | gn streamed | bn_bwd_reduce + bn_bwd_dx

A window is `iters` calls between two device events. Every round runs one
window of each arm, in turn, so the arms see the same machine; the band of
an arm is (max - min) / median over its rounds. An arm the path rule does
not serve (a tile that does not fit in registers) is reported as null.

    python benchmarks/gn_bench.py [--rounds 7] [--iters 10] [--scale 1.0]
                                  [--out results.json]

--scale shrinks the batch (for a rehearsal). Needs a GPU: there is no CPU
mode. Results: profiles/r14_groupnorm.md.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mi355x.ops import ext  # noqa: E402

SHAPES = [(8192, 32, 32, 64), (8192, 16, 16, 128), (8192, 8, 8, 256),
          (8192, 4, 4, 512), (256, 112, 112, 64)]
G, EPS = 32, 1e-5


def _window(fn, iters):
    a, b = torch.cuda.Event(True), torch.cuda.Event(True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def _serves(fn):
    try:
        fn()
    except RuntimeError as e:
        if "resident path" in str(e):
            return False
        raise
    return True


def bench_shape(N, H, W, C, rounds, iters):
    dev, bf = "cuda", torch.bfloat16
    x = torch.randn(N, H, W, C, device=dev, dtype=bf)
    res = torch.randn_like(x)
    dy = torch.randn_like(x)
    gamma = torch.rand(C, device=dev) + 0.5
    beta = torch.randn(C, device=dev)
    e16 = torch.empty(0, device=dev, dtype=bf)
    ef = torch.empty(0, device=dev)
    m = float(N * H * W)

    _, mean, rstd, mask = ext().gn_fwd(x, gamma, beta, res, G, EPS, 1, True,
                                       2, 0)
    st = ext().bn_stats(x)
    mi = ext().bn_finalize(st, ef, ef, m, 0.1, EPS)
    _, bmask = ext().bn_apply(x, mi[0], mi[1], gamma, beta, res, 1, True)

    def bn_fwd():
        s = ext().bn_stats(x)
        f = ext().bn_finalize(s, ef, ef, m, 0.1, EPS)
        ext().bn_apply(x, f[0], f[1], gamma, beta, res, 1, True)

    def bn_bwd():
        r = ext().bn_bwd_reduce(x, dy, e16, mi[0], mi[1], bmask, ef, ef)
        ext().bn_bwd_dx(x, dy, e16, mi[0], mi[1], gamma, r[0], r[1], m, True,
                        bmask, ef, ef)

    arms = {
        "fwd_res": lambda: ext().gn_fwd(x, gamma, beta, res, G, EPS, 1, True,
                                        1, 0),
        "fwd_str": lambda: ext().gn_fwd(x, gamma, beta, res, G, EPS, 1, True,
                                        2, 0),
        "fwd_bn": bn_fwd,
        "bwd_res": lambda: ext().gn_bwd(x, dy, mean, rstd, gamma, mask, G,
                                        True, 1),
        "bwd_str": lambda: ext().gn_bwd(x, dy, mean, rstd, gamma, mask, G,
                                        True, 2),
        "bwd_bn": bn_bwd,
    }
    live = {k: f for k, f in arms.items() if _serves(f)}
    for f in live.values():
        _window(f, 3)
    ms = {k: [] for k in live}
    for _ in range(rounds):
        for k, f in live.items():
            ms[k].append(_window(f, iters))
    out = {"shape": [N, H, W, C], "tensor_MiB": x.numel() * 2 / 2 ** 20}
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
        sys.exit("gn_bench: needs a GPU")
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
