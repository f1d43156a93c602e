"""Device time of ops.mlp (csrc/mlp.hip) against the routes it replaces,
bf16, M = 65536 rows, (D, F) in {(256, 1024), (384, 1536), (768, 3072)}:

  mlp_relu     ops.mlp(act="relu")
  lin_relu     fc2(fc1(x, act="relu")) through ops.linear: the same
               arithmetic on gemm_mfma_kernel, so this pair is the kernel
               comparison
  mlp_gelu     ops.mlp(act="gelu")
  torch_gelu   F.linear + F.gelu + F.linear in torch on bf16 weights
  mlp_gelu_k64 ops.mlp's kernels with the NT k-slice forced to 64 (72 KiB of
               dynamic LDS) instead of the rule's 32

Each arm runs forward ("fwd", under no_grad) and forward + backward ("fb",
torch.autograd.grad to x and the four parameters). TFLOP/s counts 4 M D F
forward and 12 M D F forward + backward over the median time.

A window is `iters` calls between two device events. Every round runs one
window of each arm, in turn, so the arms see the same machine; the band of
an arm is (max - min) / median over its rounds.

    python benchmarks/mlp_bench.py [--rounds 7] [--iters 5] [--scale 1.0]
                                   [--dims 256,384,768] [--only ARM.fb]
                                   [--out results.json]

--scale shrinks M (for a rehearsal); --only runs one arm without the timing
rounds' alternation (for a rocprofv3 --kernel-trace --stats run, which gives
that arm's kernels and launch count). Needs a GPU: there is no CPU mode.
Results: profiles/r19_mlp.md.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mi355x import ops  # noqa: E402
from mi355x.ops import functional as fn  # noqa: E402

M = 65536
HIDDEN = {256: 1024, 384: 1536, 768: 3072}


def _window(f, iters):
    a, b = torch.cuda.Event(True), torch.cuda.Event(True)
    a.record()
    for _ in range(iters):
        f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def _arms(m, D):
    Fh, bf = HIDDEN[D], torch.bfloat16
    dev = "cuda"
    x = torch.randn(m, D, device=dev, dtype=bf).requires_grad_()
    dy = torch.randn(m, D, device=dev, dtype=bf)
    w1 = (torch.randn(Fh, D, device=dev) / D ** 0.5).requires_grad_()
    w2 = (torch.randn(D, Fh, device=dev) / Fh ** 0.5).requires_grad_()
    b1 = torch.randn(Fh, device=dev).requires_grad_()
    b2 = torch.randn(D, device=dev).requires_grad_()
    p32 = [w1, b1, w2, b2]
    p16 = [t.detach().to(bf).requires_grad_() for t in p32]

    routes = {
        "mlp_relu": (lambda: ops.mlp(x, *p32, act="relu"), p32),
        "lin_relu": (lambda: ops.linear(ops.linear(x, w1, b1, "relu"),
                                        w2, b2), p32),
        "mlp_gelu": (lambda: ops.mlp(x, *p32, act="gelu"), p32),
        "torch_gelu": (lambda: F.linear(F.gelu(F.linear(x, p16[0], p16[1])),
                                        p16[2], p16[3]), p16),
        "mlp_gelu_k64": (lambda: fn._MLPFn.apply(x, *p32, 2, 64), p32),
    }

    def arm(route, params, back):
        def run():
            if not back:
                with torch.no_grad():
                    return route()
            return torch.autograd.grad(route(), [x] + params, dy)
        return run

    return {f"{name}.{'fb' if back else 'fwd'}": arm(route, params, back)
            for name, (route, params) in routes.items()
            for back in (False, True)}


def bench_dim(m, D, rounds, iters, only):
    arms = _arms(m, D)
    if only:
        arms = {only: arms[only]}
    for f in arms.values():
        _window(f, 2)
    ms = {k: [] for k in arms}
    for _ in range(rounds):
        for k, f in arms.items():
            ms[k].append(_window(f, iters))
    out = {"M": m, "D": D, "F": HIDDEN[D]}
    for k, v in ms.items():
        med = statistics.median(v)
        flop = (12 if k.endswith(".fb") else 4) * m * D * HIDDEN[D]
        out[k] = {"median_ms": round(med, 4), "min_ms": round(min(v), 4),
                  "max_ms": round(max(v), 4),
                  "band": round((max(v) - min(v)) / med, 4),
                  "TFLOPs": round(flop / med / 1e9, 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--dims", default="256,384,768")
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mlp_bench: needs a GPU")
    results = []
    for D in (int(d) for d in args.dims.split(",")):
        res = bench_dim(max(1, int(M * args.scale)), D, args.rounds,
                        args.iters, args.only)
        print(json.dumps(res), flush=True)
        results.append(res)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
