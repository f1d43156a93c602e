"""Float64 references for the kernels in csrc/bn.hip and csrc/pool.hip, and
the error bounds the GPU tests hold those kernels to.

Every function is plain torch and runs on whatever device its inputs live
on. It takes the same 16-bit (or fp32) tensors the kernel reads and upcasts
them exactly, so the only error in a reference value is float64 rounding.
tests/test_bn_pool_ref_cpu.py checks each one against torch's own float64
batch_norm / max_pool2d / mean with autograd before any kernel is judged by
it.

Layouts are the kernels': activations [..., C] channel-minor (NHWC for the
pools), per-channel vectors [C], stats [2, C].
"""

from __future__ import annotations

from typing import NamedTuple

import torch
import torch.nn.functional as F

F64 = torch.float64


# ---------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------


def u16(dtype: torch.dtype) -> float:
    """Half an ulp, relative, of a 16-bit format: the error of one rounding
    to nearest (bf16 keeps 8 significant bits, fp16 11)."""
    if dtype == torch.bfloat16:
        return 2.0 ** -8
    if dtype == torch.float16:
        return 2.0 ** -11
    raise ValueError(f"u16: not a 16-bit float dtype: {dtype}")


def fp32_sum_bound(n, terms: torch.Tensor) -> torch.Tensor:
    """Worst case of summing ``n`` fp32 terms along dim 0 in ANY order:
    (n + 4) * 2^-24 * sum|term| (n - 1 additions, each off by at most half
    an ulp of a partial sum no larger than sum|term|; +4 pays for up to four
    roundings inside a term, and the missing -1 for the second-order part).
    ``terms`` are the exact float64 terms."""
    return (n + 4) * 2.0 ** -24 * terms.abs().sum(0)


# ---------------------------------------------------------------------------
# batch norm
# ---------------------------------------------------------------------------


class BNFinalize(NamedTuple):
    mean: torch.Tensor
    var: torch.Tensor            # biased, clamped at 0
    invstd: torch.Tensor
    running_mean: torch.Tensor | None
    running_var: torch.Tensor | None
    dvar: torch.Tensor           # fp32 error budget of the kernel's var


def bn_finalize_ref(stats, rm, rv, m_total, momentum, eps) -> BNFinalize:
    """(sum, sumsq) [2,C] -> mean, invstd and the updated running stats, as
    torch's batch norm defines them: biased variance (never below 0) under
    the root, unbiased variance m/(m-1) (factor 1 for m = 1) blended into
    running_var. ``rm``/``rv`` may be None or empty: no running stats.

    dvar = 4 * 2^-24 * (sumsq/m + mean^2) bounds what an fp32 evaluation of
    sumsq/m - mean^2 can be off by: 1/m, the two products with it, mean^2
    and the subtraction round 3 times on the sumsq side and 5 on the mean^2
    side at most, 3*E2 + 4*mean^2 <= 4*(E2 + mean^2) with |var| <= E2."""
    s = stats.to(F64)
    m = float(m_total)
    mean = s[0] / m
    e2 = s[1] / m
    var = (e2 - mean * mean).clamp_min(0.0)
    invstd = torch.rsqrt(var + eps)
    dvar = 4 * 2.0 ** -24 * (e2.abs() + mean * mean)
    new_rm = new_rv = None
    if rm is not None and rm.numel() > 0:
        unbias = m / max(m - 1.0, 1.0)
        new_rm = rm.to(F64) * (1.0 - momentum) + mean * momentum
        new_rv = rv.to(F64) * (1.0 - momentum) + var * unbias * momentum
    return BNFinalize(mean, var, invstd, new_rm, new_rv, dvar)


def bn_apply_ref(x, mean, invstd, gamma, beta, res, act):
    """relu?((x - mean) * invstd * gamma + beta [+ res]) in float64, not
    rounded to 16 bits. ``res`` None or empty: no residual; ``act`` truthy:
    ReLU. Returns (value, mag) with mag = |x*sc| + |mean*sc| + |beta| +
    |res|, sc = gamma*invstd: the magnitudes an fp32 evaluation rounds at."""
    xd = x.to(F64)
    sc = gamma.to(F64) * invstd.to(F64)
    v = (xd - mean.to(F64)) * sc + beta.to(F64)
    mag = (xd * sc).abs() + (mean.to(F64) * sc).abs() + beta.to(F64).abs()
    if res is not None and res.numel() > 0:
        v = v + res.to(F64)
        mag = mag + res.to(F64).abs()
    if act:
        v = v.clamp_min(0.0)
    return v, mag


def bn_apply_bound(ref, mag, dtype):
    """|y - ref| allowed for a 16-bit y: one rounding to 16 bits, plus the
    fp32 evaluation (sc, sh = beta - mean*sc, x*sc + sh, + res: at most 3
    roundings on any one of the magnitudes, doubled to 8 * 2^-24 to cover
    the 16-bit rounding of that error and an unfused evaluation order),
    plus half the fp16 subnormal spacing."""
    b = u16(dtype) * ref.abs() + 8 * 2.0 ** -24 * mag
    if dtype == torch.float16:
        b = b + 2.0 ** -25
    return b


class BNBwd(NamedTuple):
    dx: torch.Tensor | None
    t_dgamma: torch.Tensor       # per-element terms of sum dy*xhat
    t_dbeta: torch.Tensor        # per-element terms of sum dy
    mag: torch.Tensor | None     # |g*d| + |g*dbeta/m| + |g*xhat*dgamma/m|
    d: torch.Tensor              # the masked dy (exactly a 16-bit value)


def bn_bwd_ref(x, dy, keep, mean, invstd, gamma, dgamma, dbeta,
               m_total) -> BNBwd:
    """Batch-norm backward in float64. ``keep`` (bool, x's shape, or None)
    is the ReLU mask: dy counts only where it is True. The reduction terms
    are d*xhat and d, xhat = (x - mean)*invstd; with ``dgamma``/``dbeta``
    given (else dx is None)

        dx = gamma*invstd * (d - dbeta/m - xhat*dgamma/m)."""
    d = dy.to(F64)
    if keep is not None:
        d = torch.where(keep, d, torch.zeros_like(d))
    xh = (x.to(F64) - mean.to(F64)) * invstd.to(F64)
    t_dg, t_db = d * xh, d
    if dgamma is None:
        return BNBwd(None, t_dg, t_db, None, d)
    g = gamma.to(F64) * invstd.to(F64)
    m = float(m_total)
    b = dbeta.to(F64) / m
    a = xh * (dgamma.to(F64) / m)
    dx = g * (d - b - a)
    mag = (g * d).abs() + (g * b).abs() + (g * a).abs()
    return BNBwd(dx, t_dg, t_db, mag, d)


def bn_bwd_dx_bound(ref, mag, dtype):
    """|dx - ref| allowed: one rounding to 16 bits plus the fp32 evaluation.
    The longest chain, gamma*invstd * (xhat * dgamma/m), rounds at 1/m,
    dgamma/m, x - mean, * invstd, * a, the two subtractions, gamma*invstd
    and the last product: 9 roundings, 12 * 2^-24 with the 16-bit rounding
    of that error and second-order terms."""
    b = u16(dtype) * ref.abs() + 12 * 2.0 ** -24 * mag
    if dtype == torch.float16:
        b = b + 2.0 ** -25
    return b


# ---------------------------------------------------------------------------
# pooling
# ---------------------------------------------------------------------------


def pool_out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def maxpool_ref(x, k, s, p, work=F64):
    """Max pool over NHWC. Returns (y, idx): y in x's dtype (a max of 16-bit
    values is exact) and idx uint8, the relative position r*k + c of the
    winning tap: the first, in scan order r then c, among the window's
    IN-IMAGE taps that holds the maximum. Padding never takes part. A NaN
    beats every number and the first NaN stays (torch.max_pool2d's rule).
    ``work`` is the comparison dtype; any float type that holds x exactly
    gives the same result."""
    if p > k // 2:
        raise ValueError(f"maxpool_ref: pad {p} > kernel {k} // 2")
    N, H, W, C = x.shape
    P, Q = pool_out(H, k, s, p), pool_out(W, k, s, p)
    xp = F.pad(x.to(work), (0, 0, p, p, p, p))
    inimg = F.pad(torch.ones(H, W, dtype=torch.bool, device=x.device),
                  (p, p, p, p))
    best = torch.zeros(N, P, Q, C, dtype=work, device=x.device)
    idx = torch.zeros(N, P, Q, C, dtype=torch.uint8, device=x.device)
    have = torch.zeros(1, P, Q, 1, dtype=torch.bool, device=x.device)
    for r in range(k):
        rows = slice(r, r + (P - 1) * s + 1, s)
        for c in range(k):
            cols = slice(c, c + (Q - 1) * s + 1, s)
            v = xp[:, rows, cols, :]
            ok = inimg[rows, cols][None, :, :, None]
            take = ok & (~have | (v > best)
                         | (torch.isnan(v) & ~torch.isnan(best)))
            best = torch.where(take, v, best)
            idx = torch.where(take, torch.full_like(idx, r * k + c), idx)
            have = have | ok
    assert bool(have.all())
    return best.to(x.dtype), idx


class PoolBwd(NamedTuple):
    dx: torch.Tensor      # float64 [N,H,W,C]
    abs_sum: torch.Tensor  # sum |term| per dx element
    count: torch.Tensor   # number of terms per dx element (int64)


def maxpool_bwd_ref(dy, idx, H, W, k, s, p, work=F64) -> PoolBwd:
    """Scatter-add of dy [N,P,Q,C] by relative index: window (i,j) with
    idx = r*k + c sends its dy to pixel (i*s - p + r, j*s - p + c). A tap
    that lies in the padding receives nothing here, so count.sum() equals
    dy.numel() exactly when every index names an in-image tap."""
    N, P, Q, C = dy.shape
    Hp = max((P - 1) * s + k, H + 2 * p)
    Wp = max((Q - 1) * s + k, W + 2 * p)
    dev = dy.device
    dx = torch.zeros(N, Hp, Wp, C, dtype=work, device=dev)
    ab = torch.zeros_like(dx)
    cnt = torch.zeros(N, Hp, Wp, C, dtype=torch.int64, device=dev)
    d = dy.to(work)
    zero = torch.zeros_like(d)
    for r in range(k):
        rows = slice(r, r + (P - 1) * s + 1, s)
        for c in range(k):
            cols = slice(c, c + (Q - 1) * s + 1, s)
            sel = idx == r * k + c
            # one tap's targets are distinct pixels: a plain strided add
            dx[:, rows, cols, :] += torch.where(sel, d, zero)
            ab[:, rows, cols, :] += torch.where(sel, d.abs(), zero)
            cnt[:, rows, cols, :] += sel
    crop = (slice(None), slice(p, p + H), slice(p, p + W), slice(None))
    return PoolBwd(dx[crop], ab[crop], cnt[crop])


def gap_ref(x):
    """NHWC [N,H,W,C] -> (mean over H,W, mean of |x| over H,W) in float64."""
    xd = x.to(F64)
    return xd.mean(dim=(1, 2)), xd.abs().mean(dim=(1, 2))


def gap_bwd_ref(dy, H, W):
    """[N,C] -> [N,H,W,C]: every pixel receives dy / (H*W)."""
    N, C = dy.shape
    return (dy.to(F64) / (H * W)).reshape(N, 1, 1, C).expand(N, H, W, C)
