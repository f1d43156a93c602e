"""The pooling kernels of csrc/pool.hip, element by element, against the
float64 references of _bn_pool_ref.py.

A max of 16-bit values is exact, so maxpool_fwd must return the reference's
bits and its argmax (first in scan order among in-image taps). The backward
is compared per element with the scatter-add reference: exactly where the
sums are exact in 16 bits, within one rounding plus the fp32 summation
bound otherwise. C % 8 == 0 takes the 8-channel vector kernels, any other C
the scalar ones. References are computed on the device."""

import pytest
import torch

from _bn_pool_ref import (gap_bwd_ref, gap_ref, maxpool_bwd_ref, maxpool_ref,
                          pool_out, u16)
from mi355x.ops import functional as fn
from mi355x.ops._ext import ext

pytestmark = pytest.mark.gpu

F64 = torch.float64
DTYPES = [torch.bfloat16, torch.float16]
GEOMS = [(2, 2, 0), (3, 2, 1), (3, 1, 1), (3, 3, 0),
         (2, 3, 0),            # gaps between windows
         (5, 2, 2)]
SIZES = [(7, 9), (8, 8), (10, 6)]   # the floor drops a row or a column
N = 3
CS = [8, 16, 3, 6]             # vector path, vector path, scalar, scalar
KINDS = ["normal", "ties", "negative"]
GRID_CAP = 16384 * 256         # work items of one grid stride (pgrid)


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _x(kind, H, W, C, dtype, seed):
    g = _gen(seed)
    shape = (N, H, W, C)
    if kind == "normal":
        x = torch.randn(shape, generator=g, device="cuda")
    elif kind == "ties":       # ties everywhere: the first-index rule decides
        x = torch.randint(-3, 4, shape, generator=g, device="cuda").float()
    else:                      # all negative: padding must never win
        x = -torch.rand(shape, generator=g, device="cuda") - 0.25
    return x.to(dtype)


def _dy_exact(shape, dtype, seed):
    """{-4..4}/4: every sum of up to 9 terms is exact in bf16 and fp16."""
    return (torch.randint(-4, 5, shape, generator=_gen(seed), device="cuda")
            / 4.0).to(dtype)


def _cases(k, s, p, C, dtype):
    for H, W in SIZES:
        for i, kind in enumerate(KINDS):
            yield H, W, _x(kind, H, W, C, dtype, seed=H * 100 + W + i)


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("k,s,p", GEOMS)
def test_maxpool_fwd_exact(k, s, p, C, dtype):
    for H, W, x in _cases(k, s, p, C, dtype):
        y, idx = ext().maxpool_fwd(x, k, s, p)
        yr, ir = maxpool_ref(x, k, s, p)
        assert y.shape == (N, pool_out(H, k, s, p), pool_out(W, k, s, p), C)
        assert y.dtype == dtype and idx.dtype == torch.uint8
        assert torch.equal(_bits(y), _bits(yr)), (H, W)
        assert torch.equal(idx, ir), (H, W)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("k,s,p", GEOMS)
def test_maxpool_bwd_elementwise(k, s, p, C, dtype):
    for H, W, x in _cases(k, s, p, C, dtype):
        y, idx = ext().maxpool_fwd(x, k, s, p)
        # exact: small dyadic dy
        dy = _dy_exact(y.shape, dtype, seed=H + W + k)
        dx = ext().maxpool_bwd(dy, idx, H, W, k, s, p)
        ref = maxpool_bwd_ref(dy, idx, H, W, k, s, p)
        assert int(ref.count.sum()) == dy.numel()   # every idx is in-image
        assert int(ref.count.max()) <= 9
        assert dx.shape == x.shape and dx.dtype == dtype
        assert torch.equal(dx.to(F64), ref.dx), (H, W)
        # random normal dy: one rounding to 16 bits, and n fp32 additions
        dy = torch.randn(y.shape, generator=_gen(H * W + s),
                         device="cuda").to(dtype)
        dx = ext().maxpool_bwd(dy, idx, H, W, k, s, p)
        ref = maxpool_bwd_ref(dy, idx, H, W, k, s, p)
        bound = (u16(dtype) * ref.dx.abs()
                 + ref.count * 2.0 ** -24 * ref.abs_sum)
        if dtype == torch.float16:
            bound = bound + 2.0 ** -25          # fp16 subnormal spacing
        err = (dx.to(F64) - ref.dx).abs()
        assert bool((err <= bound).all()), (H, W, float((err - bound).max()))
        # pixels no window chose get an exact zero
        assert bool((dx[ref.count == 0] == 0).all())


@pytest.mark.parametrize("C,HW", [(3, 1366), (8, 2366)])
def test_maxpool_grid_stride(C, HW):
    """Just over 16384*256 work items in the forward (and several strides
    in the backward): the stride loop of each path. A float32 reference is
    exact for a max and for these sums of at most 4 small dyadic terms."""
    k, s, p = 3, 2, 1
    dtype = torch.bfloat16
    P = pool_out(HW, k, s, p)
    items = N * P * P * (C // 8 if C % 8 == 0 else C)
    assert GRID_CAP < items < GRID_CAP + GRID_CAP // 256
    x = torch.randn(N, HW, HW, C, generator=_gen(C), device="cuda").to(dtype)
    y, idx = ext().maxpool_fwd(x, k, s, p)
    yr, ir = maxpool_ref(x, k, s, p, work=torch.float32)
    assert torch.equal(_bits(y), _bits(yr))
    assert torch.equal(idx, ir)
    del yr, ir
    dy = _dy_exact(y.shape, dtype, seed=C + 1)
    dx = ext().maxpool_bwd(dy, idx, HW, HW, k, s, p)
    ref = maxpool_bwd_ref(dy, idx, HW, HW, k, s, p, work=torch.float32)
    assert int(ref.count.sum()) == dy.numel()
    assert torch.equal(dx.float(), ref.dx)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [8, 3])
def test_maxpool_nonfinite(C, dtype):
    """torch.max_pool2d's rules: a window holding a NaN gives NaN, idx names
    the in-image tap that holds it and the backward routes dy there; a
    window of all -inf gives -inf (no sentinel); +inf wins."""
    k, s, p = 3, 2, 1
    H = W = 8
    nan, inf = float("nan"), float("inf")
    x = _x("normal", H, W, C, dtype, seed=5)
    # one NaN per (n, c) plane at most, so no window holds two: at an odd
    # pixel (four windows, a different tap of each), an even one, two corners
    x[0, 3, 5, 0] = nan
    x[1, 4, 2, 1] = nan
    x[2, 0, 0, 2] = nan
    x[2, 7, 7, 0] = nan
    x[0, 0:3, 0:3, 2] = -inf      # window (0,0), rows/cols 0..1: all -inf
    x[1, 0:2, 5:8, 2] = -inf      # window (0,3), cols 5..7
    x[1, 5, 5, 0] = inf
    x[0, 6, 1, 1] = inf
    y, idx = ext().maxpool_fwd(x, k, s, p)
    yr, ir = maxpool_ref(x, k, s, p)
    assert int(torch.isnan(yr).sum()) == 4 + 1 + 1 + 1
    assert torch.equal(torch.isnan(y), torch.isnan(yr))
    ok = ~torch.isnan(yr)
    assert torch.equal(_bits(y)[ok], _bits(yr)[ok])
    assert y[0, 0, 0, 2] == -inf and y[1, 0, 3, 2] == -inf
    assert int((y == inf).sum()) == int((yr == inf).sum()) >= 3
    # at most one NaN per window, so "a tap holding a NaN" is one tap
    assert torch.equal(idx, ir)
    dy = _dy_exact(y.shape, dtype, seed=9)
    dx = ext().maxpool_bwd(dy, idx, H, W, k, s, p)
    ref = maxpool_bwd_ref(dy, idx, H, W, k, s, p)
    assert int(ref.count.sum()) == dy.numel()
    assert torch.equal(dx.to(F64), ref.dx)
    # the NaN at pixel (3,5) of plane (0, 0) gets the dy of its 4 windows
    assert ref.count[0, 3, 5, 0] == 4
    assert dx[0, 3, 5, 0].to(F64) == dy[0, 1:3, 2:4, 0].to(F64).sum()


@pytest.mark.parametrize("k,p", [(3, 2), (2, 2), (5, 3)])
def test_maxpool_rejects_pad_over_half_kernel(k, p):
    x = torch.zeros(1, 8, 8, 8, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError) as e:
        ext().maxpool_fwd(x, k, 2, p)
    assert f"pad {p}" in str(e.value) and f"kernel size {k}" in str(e.value)
    P = pool_out(8, k, 2, p)
    dy = torch.zeros(1, P, P, 8, device="cuda", dtype=torch.bfloat16)
    idx = torch.zeros(1, P, P, 8, device="cuda", dtype=torch.uint8)
    with pytest.raises(RuntimeError) as e:
        ext().maxpool_bwd(dy, idx, 8, 8, k, 2, p)
    assert f"pad {p}" in str(e.value) and f"kernel size {k}" in str(e.value)
    # the largest legal padding still runs
    ext().maxpool_fwd(x, k, 2, k // 2)


GAP_SHAPES = [(3, 4, 4, 512), (2, 7, 7, 10), (5, 1, 1, 24),
              (2049, 1, 1, 2048)]   # N*C just past the launch cap: stride loop


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", GAP_SHAPES)
def test_global_avg_pool_fwd(shape, dtype):
    n, H, W, C = shape
    if n == 2049:
        assert GRID_CAP < n * C < GRID_CAP + GRID_CAP // 256
    x = torch.randn(shape, generator=_gen(H + C), device="cuda").to(dtype)
    y = ext().global_avg_pool(x)
    assert y.shape == (n, C) and y.dtype == dtype
    ref, absmean = gap_ref(x)
    # one rounding to 16 bits; HW - 1 fp32 additions, the division and the
    # conversion of HW: (HW + 1) * 2^-24 * sum|x| / HW
    bound = u16(dtype) * ref.abs() + (H * W + 1) * 2.0 ** -24 * absmean
    if dtype == torch.float16:
        bound = bound + 2.0 ** -25
    err = (y.to(F64) - ref).abs()
    assert bool((err <= bound).all()), float((err / bound).max())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", GAP_SHAPES[:3])
def test_global_avg_pool_bwd(shape, dtype):
    n, H, W, C = shape
    x = torch.randn(shape, generator=_gen(C), device="cuda").to(dtype)
    x.requires_grad_(True)
    y = fn.global_avg_pool(x)
    dy = torch.randn(n, C, generator=_gen(C + 1), device="cuda").to(dtype)
    y.backward(dy)
    ref = gap_bwd_ref(dy, H, W)
    assert x.grad.shape == x.shape and x.grad.dtype == dtype
    bound = u16(dtype) * ref.abs()
    if dtype == torch.float16:
        bound = bound + 2.0 ** -25
    err = (x.grad.to(F64) - ref).abs()
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())
