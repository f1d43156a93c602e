"""Device time of ops.layer_norm (csrc/ln.hip) against the two other routes
to the same result, bf16, M = 65536 rows, D in {256, 384, 768, 1024}:

  ln     ops.layer_norm, plain and with the fused residual add
  gn     the group_norm view [M,1,1,D] with one group plus an eager add: the
         route layers.LayerNorm took before; only where D is a power of two
  torch  F.layer_norm plus an eager add
  ln_nv4 at D = 256 only: the kernel forced to 8 lanes x 4 vectors instead
         of the rule's 32 x 1

Each arm runs forward ("fwd") and forward + backward ("fb") through
autograd; the fused form ("add") returns (s, y) and takes a gradient on
both. GB/s is the op's minimum traffic over the median time: with E = M*D
elements of 2 bytes, fwd moves 2E (x, y), fwd add 4E (x, r, s, y), the
backward adds 3E (s, dy, d) or 4E with ds.

A window is `iters` calls between two device events. Every round runs one
window of each arm, in turn, so the arms see the same machine; the band of
an arm is (max - min) / median over its rounds.

    python benchmarks/ln_bench.py [--rounds 7] [--iters 10] [--scale 1.0]
                                  [--out results.json]

--scale shrinks M (for a rehearsal). Needs a GPU: there is no CPU mode.
Results: profiles/r18_layernorm.md.
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

M, DIMS, EPS = 65536, (256, 384, 768, 1024), 1e-5
ELEMS = {"fwd": 2, "fwd_add": 4, "fb": 5, "fb_add": 8}  # times E, 2 bytes


def _window(f, iters):
    a, b = torch.cuda.Event(True), torch.cuda.Event(True)
    a.record()
    for _ in range(iters):
        f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def _routes(D):
    """route -> f(x, r or None, gamma, beta) returning y or (s, y)"""
    def gn(x, r, g, b):
        s = x if r is None else x + r
        y = ops.group_norm(s.view(-1, 1, 1, D), 1, g, b, None, None, EPS)
        return y.view(s.shape) if r is None else (s, y.view(s.shape))

    def eager(x, r, g, b):
        s = x if r is None else x + r
        y = F.layer_norm(s, (D,), g.to(s.dtype), b.to(s.dtype), EPS)
        return y if r is None else (s, y)

    routes = {"ln": lambda x, r, g, b: ops.layer_norm(x, g, b, r, EPS),
              "torch": eager}
    if D & (D - 1) == 0:
        routes["gn"] = gn
    if D == 256:
        routes["ln_nv4"] = lambda x, r, g, b: fn._LNFn.apply(x, g, b, r, EPS,
                                                             4)
    return routes


def bench_dim(m, D, rounds, iters):
    bf = torch.bfloat16
    x, r, dy, ds = (torch.randn(m, D, device="cuda", dtype=bf)
                    for _ in range(4))
    gamma = torch.rand(D, device="cuda") + 0.5
    beta = torch.randn(D, device="cuda")
    leaves = [t.requires_grad_() for t in (x, r, gamma, beta)]

    def arm(route, add, back):
        def run():
            if not back:
                with torch.no_grad():
                    return route(x, r if add else None, gamma, beta)
            out = route(x, r if add else None, gamma, beta)
            ins = leaves if add else [x, gamma, beta]
            return torch.autograd.grad(out, ins, (ds, dy) if add else dy)
        return run

    arms = {f"{name}.{'fb' if back else 'fwd'}{'_add' if add else ''}":
            arm(route, add, back)
            for name, route in _routes(D).items()
            for back in (False, True) for add in (False, True)}
    for f in arms.values():
        _window(f, 3)
    ms = {k: [] for k in arms}
    for _ in range(rounds):
        for k, f in arms.items():
            ms[k].append(_window(f, iters))
    out = {"M": m, "D": D, "tensor_MiB": m * D * 2 / 2 ** 20}
    for k, v in ms.items():
        med = statistics.median(v)
        nbytes = ELEMS[k.split(".")[1]] * m * D * 2
        out[k] = {"median_ms": round(med, 4), "min_ms": round(min(v), 4),
                  "max_ms": round(max(v), 4),
                  "band": round((max(v) - min(v)) / med, 4),
                  "GBps": round(nbytes / med / 1e6, 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ln_bench: needs a GPU")
    results = []
    for D in DIMS:
        res = bench_dim(max(1, int(M * args.scale)), D, args.rounds,
                        args.iters)
        print(json.dumps(res), flush=True)
        results.append(res)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
