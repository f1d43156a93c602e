"""Device time of ops.attention (csrc/attn.hip, S <= 256) and of
ops.flash_attention (csrc/attn_flash.hip, S <= 4096) against two torch
comparators on the same values, from and to the packed qkv layout:

  fused     ops.attention up to 256 tokens, ops.flash_attention above: what
            layers.MultiHeadAttention calls
  flash     ops.flash_attention where fused is the resident op (197x8x64 and
            256x4x32 only): the measurement behind the layer's crossover
  sdpa      F.scaled_dot_product_attention, with the permute copies it needs
            from [B,S,3,H,dh] and back to [B,S,D]
  composed  torch.matmul, softmax, torch.matmul, the same copies

Shapes (S, H, dh), bf16: 64x4x64 (vit_cifar), 197x8x64, 256x4x32 at batch
--batch; 577x6x64 at --batch / 8, 784x6x64 (vit_s8) and 1024x4x32 at
--batch / 16, 4096x4x64 at --batch / 128, so that the composed arm's S^2
scores fit.

  fwd_*  forward only, under no_grad
  fb_*   forward + backward into qkv.grad

A window is `iters` calls between two device events. Every round runs one
window of each arm, in turn, so the arms see the same machine; the band of
an arm is (max - min) / median over its rounds. Bytes are the HBM traffic
the fused op needs (forward: qkv in, o and lse out; backward adds qkv, lse
and do in, dqkv out); FLOPs count two per multiply-add of the matrix
products (forward 4 S^2 dh, backward 10 S^2 dh a head: the fused backward
forms S and dP twice, which is not counted).

    python benchmarks/attn_bench.py [--batch 1024] [--rounds 7] [--iters 10]
                                    [--out results.json]

Needs a GPU: there is no CPU mode. Results: profiles/r17_attention.md and
profiles/r21_flash_attention.md.
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

import mi355x.ops as ops  # noqa: E402

# (S, H, dh, batch divisor, also time ops.flash_attention)
SHAPES = [(64, 4, 64, 1, False), (197, 8, 64, 1, True), (256, 4, 32, 1, True),
          (577, 6, 64, 8, False), (784, 6, 64, 16, False),
          (1024, 4, 32, 16, False), (4096, 4, 64, 128, False)]


def _window(f, iters):
    a, b = torch.cuda.Event(True), torch.cuda.Event(True)
    a.record()
    for _ in range(iters):
        f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def _heads(qkv):
    return (qkv[:, :, i].permute(0, 2, 1, 3).contiguous() for i in range(3))


def _sdpa(qkv, H):
    B, S = qkv.shape[:2]
    q, k, v = _heads(qkv)
    o = F.scaled_dot_product_attention(q, k, v)
    return o.permute(0, 2, 1, 3).reshape(B, S, -1)


def _composed(qkv, H):
    B, S = qkv.shape[:2]
    q, k, v = _heads(qkv)
    p = torch.softmax(torch.matmul(q, k.transpose(-1, -2))
                      * q.shape[-1] ** -0.5, dim=-1)
    return torch.matmul(p, v).permute(0, 2, 1, 3).reshape(B, S, -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "attn_bench needs a GPU"
    results = []
    for S, H, dh, div, both in SHAPES:
        B = max(1, args.batch // div)
        g = torch.Generator().manual_seed(S)
        qkv = torch.randn(B, S, 3, H, dh, generator=g).bfloat16().cuda()
        dy = torch.randn(B, S, H * dh, generator=g).bfloat16().cuda()
        leaf = qkv.clone().requires_grad_()
        op = ops.attention if S <= 256 else ops.flash_attention
        impls = {"fused": lambda t: op(t, H),
                 "sdpa": lambda t: _sdpa(t, H),
                 "composed": lambda t: _composed(t, H)}
        if both:
            impls["flash"] = lambda t: ops.flash_attention(t, H)
        arms = {}
        for name, f in impls.items():
            def fwd(f=f):
                with torch.no_grad():
                    f(qkv)

            def fb(f=f):
                leaf.grad = None
                f(leaf).backward(dy)

            arms["fwd_" + name], arms["fb_" + name] = fwd, fb
        for f in arms.values():  # warm up every arm at this shape
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        for _ in range(args.rounds):
            for k, f in arms.items():
                times[k].append(_window(f, args.iters))
        e = B * S * H * dh  # elements of q (= k = v = o)
        fwd_bytes = 2 * 4 * e + 4 * B * H * S
        bwd_bytes = 2 * 7 * e + 4 * B * H * S
        fwd_flops = 4 * B * H * S * S * dh
        row = {"B": B, "S": S, "H": H, "dh": dh, "fwd_bytes": fwd_bytes,
               "fb_bytes": fwd_bytes + bwd_bytes, "fwd_flops": fwd_flops,
               "fb_flops": fwd_flops * 7 // 2}
        for k, ts in times.items():
            med = statistics.median(ts)
            row[k] = {"ms": round(med, 4),
                      "band": round((max(ts) - min(ts)) / med, 3)}
        for d in ("fwd", "fb"):
            ms = row[d + "_fused"]["ms"]
            row[d + "_fused"]["GB/s"] = round(row[d + "_bytes"] / ms / 1e6, 1)
            row[d + "_fused"]["TFLOP/s"] = round(
                row[d + "_flops"] / ms / 1e9, 2)
            row[d + "_vs_sdpa"] = round(row[d + "_sdpa"]["ms"] / ms, 3)
            if both:
                row[d + "_flash_vs_fused"] = round(
                    ms / row[d + "_flash"]["ms"], 3)
        print(json.dumps(row), flush=True)
        results.append(row)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
