"""Each batch-norm entry point of csrc/bn.hip on its own, through ext(),
against the float64 references and derived bounds of _bn_pool_ref.py.

Fast path (bn_*_fast, bn_reduce_fast): C % 8 == 0 and 2048 % C == 0.
Everything else takes the fallback kernels: C = 40 is a multiple of 8 that
is not fast, C = 300 needs two channel blocks. M is small and ragged except
where a grid-stride boundary is the point. References are computed on the
device in float64; every element takes part in every comparison."""

import pytest
import torch

from _bn_pool_ref import (bn_apply_bound, bn_apply_ref, bn_bwd_dx_bound,
                          bn_bwd_ref, bn_finalize_ref, fp32_sum_bound)
from mi355x.ops import functional as fn
from mi355x.ops._ext import ext

pytestmark = pytest.mark.gpu

F64 = torch.float64
EPS = 1e-5
FAST_C = [8, 64, 512, 2048]
SLOW_C = [6, 40, 300]
MS = [37, 700]
DTYPES = [torch.bfloat16, torch.float16]
# bn_apply_fast / bn_bwd_dx_fast cover 2048*256*8 elements per grid stride
STRIDE = 2048 * 256 * 8
BOUNDARY = [(64, 65576),    # E just above 1 stride: paired step or tail
            (2048, 6147)]   # just above 3: paired step, then tail


def _fast(C):
    return C % 8 == 0 and 2048 % C == 0


def _e(dtype=torch.float32):
    return torch.empty(0, device="cuda", dtype=dtype)


def _inputs(C, M, dtype, seed=0):
    """x, res, dy [M,C] in ``dtype``; mean, invstd, gamma, beta [C] fp32.
    Channel 0 and the last have a negative gamma; channel 1 is the
    tiny-variance case (x within a few 16-bit steps of its mean, invstd
    near 1/sqrt(eps))."""
    g = torch.Generator(device="cuda").manual_seed(seed * 7919 + C + M)

    def rn(*s):
        return torch.randn(*s, generator=g, device="cuda")

    x = rn(M, C) * 2 + 0.5
    mean = 0.5 + 0.3 * rn(C)
    invstd = torch.rand(C, generator=g, device="cuda") + 0.5
    x[:, 1] = 0.5 + 0.004 * rn(M)
    mean[1] = 0.5003
    invstd[1] = (1e-5 + 1.6e-5) ** -0.5
    gamma = torch.rand(C, generator=g, device="cuda") + 0.5
    gamma[0] = -0.8
    gamma[C - 1] = -1.25
    beta = 0.1 * rn(C)
    return (x.to(dtype), rn(M, C).to(dtype), rn(M, C).to(dtype), mean, invstd,
            gamma, beta)


def _assert_within(got, ref, bound, what):
    err = (got.to(F64) - ref).abs()
    bad = err > bound
    assert not bool(bad.any()), (
        f"{what}: {int(bad.sum())} of {bad.numel()} over the bound, worst "
        f"ratio {float((err / bound.clamp_min(1e-300)).max()):.3g}")
    return float((err / bound.clamp_min(1e-300)).max())


def _mask_bits(y):
    """The packed map bn_apply stores: bit u of byte e>>3 is y[e+u] > 0."""
    w = (1 << torch.arange(8, device=y.device)).to(torch.int32)
    bits = (y.reshape(-1, 8).float() > 0).to(torch.int32)
    return (bits * w).sum(1).to(torch.uint8)


# ---------------------------------------------------------------------------
# bn_finalize
# ---------------------------------------------------------------------------


def _hand_stats(C, m_total, seed):
    """[2,C] fp32 (sum, sumsq) of channels with mean ~ N(0, 2^2) and
    variance in [0.5, 2): far from the cancellation regime."""
    g = torch.Generator().manual_seed(seed)
    mean = torch.randn(C, generator=g, dtype=F64) * 2
    var = torch.rand(C, generator=g, dtype=F64) * 1.5 + 0.5
    return torch.stack([mean * m_total,
                        (var + mean * mean) * m_total]).float().cuda()


def _check_finalize(stats, m_total, momentum, rm0, rv0):
    rm, rv = rm0.clone(), rv0.clone()
    out = ext().bn_finalize(stats, rm, rv, float(m_total), momentum, EPS)
    assert out.shape == stats.shape and out.dtype == torch.float32
    ref = bn_finalize_ref(stats, rm0, rv0, m_total, momentum, EPS)
    u = 2.0 ** -24
    # mean = sum * fl(1/m): two roundings, one more unit for second order
    _assert_within(out[0], ref.mean, 3 * u * ref.mean.abs(), "mean")
    # var is within dvar of the float64 value and never below 0; rsqrtf and
    # the addition of eps are good to 2^-20 relative with room to spare
    lo = torch.rsqrt(ref.var + ref.dvar + EPS) * (1 - 2.0 ** -20)
    hi = torch.rsqrt((ref.var - ref.dvar).clamp_min(0) + EPS) * (1 + 2.0 ** -20)
    inv = out[1].to(F64)
    assert bool(torch.isfinite(inv).all())
    assert bool((inv >= lo).all() and (inv <= hi).all()), (
        (lo - inv).max().item(), (inv - hi).max().item())
    if rm0.numel() == 0:
        return out, ref
    # r*(1-mom) + v*mom: (1-mom) and the product round 3 times with mom's own
    # rounding, v*mom 4 times (v carries 2), the sum once: 6 units in all
    unbias = m_total / max(m_total - 1.0, 1.0)
    keep = (rm0.to(F64) * (1 - momentum)).abs()
    _assert_within(rm, ref.running_mean,
                   6 * u * (keep + (ref.mean * momentum).abs()) + 1e-300,
                   "running_mean")
    keep = (rv0.to(F64) * (1 - momentum)).abs()
    blend = ref.var * unbias * momentum
    _assert_within(rv, ref.running_var,
                   ref.dvar * unbias * momentum
                   + 6 * u * (keep + blend.abs()) + 1e-300, "running_var")
    return out, ref


@pytest.mark.parametrize("momentum", [0.1, 1.0])
@pytest.mark.parametrize("m_total", [1, 2, 259, 5000])
@pytest.mark.parametrize("C", [8, 300])
def test_bn_finalize(C, m_total, momentum):
    stats = _hand_stats(C, m_total, seed=C + m_total)
    g = torch.Generator().manual_seed(1)
    rm0 = torch.randn(C, generator=g).cuda()
    rv0 = (torch.rand(C, generator=g) + 0.5).cuda()
    _check_finalize(stats, m_total, momentum, rm0, rv0)


def test_bn_finalize_without_running_stats():
    """Empty running tensors: nothing is written, same mean/invstd."""
    C, m = 40, 259
    stats = _hand_stats(C, m, seed=3)
    out, _ = _check_finalize(stats, m, 0.1, _e(), _e())
    rm, rv = torch.zeros(C).cuda(), torch.ones(C).cuda()
    assert torch.equal(ext().bn_finalize(stats, rm, rv, float(m), 0.1, EPS),
                       out)


@pytest.mark.parametrize("momentum", [0.1, 1.0])
@pytest.mark.parametrize("value,m_total", [(100.5, 5000), (250.0, 259),
                                           (64.0, 5000)])
def test_bn_finalize_constant_channel(value, m_total, momentum):
    """Stats of a constant channel (the fp32-rounded exact sums): the true
    variance is 0, and sumsq/m - mean^2 in fp32 is cancellation noise of
    either sign, far larger than eps. invstd must stay finite, between
    rsqrt(eps + dvar) and rsqrt(eps), and running_var must not go
    negative."""
    C = 8
    s = torch.tensor([value * m_total, value * value * m_total], dtype=F64)
    stats = s.float().reshape(2, 1).repeat(1, C).cuda()
    rm, rv = torch.zeros(C).cuda(), torch.zeros(C).cuda()
    out = ext().bn_finalize(stats, rm, rv, float(m_total), momentum, EPS)
    sd = stats.to(F64)
    mean = sd[0] / m_total
    dvar = 4 * 2.0 ** -24 * (sd[1] / m_total + mean * mean)
    inv = out[1].to(F64)
    print(f"value {value} m {m_total}: invstd {out[1][0].item()} "
          f"running_var {rv[0].item()} dvar {dvar[0].item():.3g}")
    assert bool(torch.isfinite(inv).all()), inv
    lo = torch.rsqrt(EPS + dvar) * (1 - 2.0 ** -20)
    hi = EPS ** -0.5 * (1 + 2.0 ** -20)
    assert bool((inv >= lo).all() and (inv <= hi).all()), inv
    assert bool((rv >= 0).all()), rv
    unbias = m_total / (m_total - 1.0)
    assert bool((rv.to(F64) <= dvar * unbias * momentum * (1 + 2.0 ** -20)).all())
    assert bool(torch.isfinite(rm).all())


# ---------------------------------------------------------------------------
# bn_apply
# ---------------------------------------------------------------------------


def _check_apply(C, M, dtype, res, act, want_mask):
    x, r, _, mean, invstd, gamma, beta = _inputs(C, M, dtype)
    rarg = r if res else _e(dtype)
    y, mask = ext().bn_apply(x, mean, invstd, gamma, beta, rarg, int(act),
                             want_mask)
    assert y.shape == x.shape and y.dtype == dtype
    ref, mag = bn_apply_ref(x, mean, invstd, gamma, beta, rarg, act)
    _assert_within(y, ref, bn_apply_bound(ref, mag, dtype), "y")
    if act:
        assert bool((y == 0).any()) and bool((y > 0).any())
    if act and want_mask and _fast(C):
        assert mask.dtype == torch.uint8 and mask.shape == (M * C // 8,)
        assert torch.equal(mask, _mask_bits(y))
    else:
        assert mask is None or mask.numel() == 0
    return y, mask


@pytest.mark.parametrize("res,act,want_mask", [
    (False, False, False), (True, False, True), (False, True, True),
    (True, True, True), (True, True, False)])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", FAST_C + SLOW_C)
def test_bn_apply(C, dtype, res, act, want_mask):
    for M in MS:
        _check_apply(C, M, dtype, res, act, want_mask)


@pytest.mark.parametrize("C,M", BOUNDARY)
def test_bn_apply_grid_stride_boundary(C, M):
    E = M * C
    assert 0 < E % STRIDE < STRIDE // 64 and E // STRIDE in (1, 3)
    _check_apply(C, M, torch.bfloat16, True, True, True)


# ---------------------------------------------------------------------------
# bn_bwd_reduce
# ---------------------------------------------------------------------------


def _check_reduce(x, dy, keep, mean, invstd, call):
    M, C = x.shape
    r = call()
    assert r.shape == (2, C) and r.dtype == torch.float32
    ref = bn_bwd_ref(x, dy, keep, mean, invstd, None, None, None, M)
    for got, terms, what in ((r[0], ref.t_dgamma, "sum dy*xhat"),
                             (r[1], ref.t_dbeta, "sum dy")):
        _assert_within(got, terms.sum(0),
                       fp32_sum_bound(M, terms) + 1e-300, what)
    assert torch.equal(call(), r)        # fixed fold order: same bits


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", FAST_C)
def test_bn_bwd_reduce_stored_mask(C, dtype):
    for M in MS:
        x, res, dy, mean, invstd, gamma, beta = _inputs(C, M, dtype)
        y, mask = ext().bn_apply(x, mean, invstd, gamma, beta, res, 1, True)
        keep = y > 0
        assert bool(keep.any()) and not bool(keep.all())
        _check_reduce(x, dy, keep, mean, invstd,
                      lambda: ext().bn_bwd_reduce(x, dy, y, mean, invstd,
                                                  mask, _e(), _e()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", SLOW_C)
def test_bn_bwd_reduce_y_mask_fallback(C, dtype):
    for M in MS + [3000]:                # 3000 rows: three chunks to fold
        x, res, dy, mean, invstd, gamma, beta = _inputs(C, M, dtype)
        y, mask = ext().bn_apply(x, mean, invstd, gamma, beta, res, 1, True)
        assert mask is None or mask.numel() == 0
        keep = y > 0
        assert bool(keep.any()) and not bool(keep.all())
        _check_reduce(x, dy, keep, mean, invstd,
                      lambda: ext().bn_bwd_reduce(x, dy, y, mean, invstd,
                                                  _e(torch.uint8), _e(),
                                                  _e()))


@pytest.mark.parametrize("C", FAST_C + SLOW_C)
def test_bn_bwd_reduce_unmasked_fp16(C):
    for M in MS:
        x, _, dy, mean, invstd, _, _ = _inputs(C, M, torch.float16)
        _check_reduce(x, dy, None, mean, invstd,
                      lambda: ext().bn_bwd_reduce(x, dy, _e(torch.float16),
                                                  mean, invstd,
                                                  _e(torch.uint8), _e(),
                                                  _e()))


def _recompute_inputs(C, M, dtype, seed=0):
    """x on the grid j/16, |j| <= 128 (exact in both 16-bit types); asc in
    +-{1, 1.5} * 2^k, k in {-1, 0, 1}; ash = -asc * x0 with x0 on the same
    grid. Every x*asc + ash is then a multiple of 2^-6 below 2^6: exact in
    fp32 whether or not the compiler fuses the multiply-add, so `> 0` has
    one answer. Row 0 holds x0 itself (the value exactly 0: masked).
    Channels 6..11 of every 12 have a negative asc."""
    g = torch.Generator(device="cuda").manual_seed(seed + C * 31 + M)
    x = torch.randint(-128, 129, (M, C), generator=g, device="cuda") / 16.0
    ci = torch.arange(C, device="cuda")
    asc = (torch.tensor([1.0, 1.5], device="cuda")[ci % 2]
           * 2.0 ** ((ci // 2) % 3 - 1).float())
    asc = torch.where((ci // 6) % 2 == 1, -asc, asc)
    x0 = torch.randint(-24, 25, (C,), generator=g, device="cuda") / 16.0
    x[0] = x0
    ash = -asc * x0
    assert bool((asc < 0).any()) and bool((asc > 0).any())
    z = x.to(F64) * asc.to(F64) + ash.to(F64)
    assert torch.equal(z * 64, (z * 64).round()) and float(z.abs().max()) < 64
    assert bool((z[0] == 0).all())
    keep = z > 0
    assert bool(keep.any()) and not bool(keep.all())
    return x.to(dtype), asc, ash, keep


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", FAST_C)
def test_bn_bwd_reduce_mask_recompute(C, dtype):
    for M in MS:
        _, _, dy, mean, invstd, _, _ = _inputs(C, M, dtype)
        x, asc, ash, keep = _recompute_inputs(C, M, dtype)
        assert torch.equal(x.to(F64) * 16, (x.to(F64) * 16).round())
        invstd[1] = 0.75     # x spans +-8 here: no tiny-variance channel
        _check_reduce(x, dy, keep, mean, invstd,
                      lambda: ext().bn_bwd_reduce(x, dy, _e(dtype), mean,
                                                  invstd, _e(torch.uint8),
                                                  asc, ash))


@pytest.mark.parametrize("C", SLOW_C)
def test_bn_mask_recompute_needs_fast_shape(C):
    M = 37
    x, _, dy, mean, invstd, gamma, _ = _inputs(C, M, torch.bfloat16)
    asc, ash = torch.ones(C).cuda(), torch.zeros(C).cuda()
    with pytest.raises(RuntimeError, match="fast BN path"):
        ext().bn_bwd_reduce(x, dy, _e(torch.bfloat16), mean, invstd,
                            _e(torch.uint8), asc, ash)
    with pytest.raises(RuntimeError, match="fast BN path"):
        ext().bn_bwd_dx(x, dy, _e(torch.bfloat16), mean, invstd, gamma,
                        torch.zeros(C).cuda(), torch.zeros(C).cuda(),
                        float(M), False, _e(torch.uint8), asc, ash)


# ---------------------------------------------------------------------------
# bn_bwd_dx
# ---------------------------------------------------------------------------


def _check_dx(C, M, dtype, variant, m_factor):
    x, res, dy, mean, invstd, gamma, beta = _inputs(C, M, dtype)
    g = torch.Generator(device="cuda").manual_seed(C + 5)
    # arbitrary reduced terms, of the size sums over M rows have
    dgamma = torch.randn(C, generator=g, device="cuda") * M ** 0.5
    dbeta = torch.randn(C, generator=g, device="cuda") * M ** 0.5
    y_arg, mask, asc, ash, keep = _e(dtype), _e(torch.uint8), _e(), _e(), None
    if variant in ("mask", "y"):
        y, m = ext().bn_apply(x, mean, invstd, gamma, beta, res, 1, True)
        keep = y > 0
        y_arg = y
        if variant == "mask":
            mask = m
        else:
            assert m is None or m.numel() == 0
    elif variant == "recompute":
        x, asc, ash, keep = _recompute_inputs(C, M, dtype)
        invstd[1] = 0.75     # x spans +-8 here: no tiny-variance channel
    m_total = float(m_factor * M)
    dx, dres = ext().bn_bwd_dx(x, dy, y_arg, mean, invstd, gamma, dgamma,
                               dbeta, m_total, True, mask, asc, ash)
    ref = bn_bwd_ref(x, dy, keep, mean, invstd, gamma, dgamma, dbeta, m_total)
    assert dx.shape == x.shape and dx.dtype == dtype
    _assert_within(dx, ref.dx, bn_bwd_dx_bound(ref.dx, ref.mag, dtype), "dx")
    # dres is the masked dy itself, bit for bit
    want = dy if keep is None else torch.where(keep, dy, torch.zeros_like(dy))
    assert dres.dtype == dtype
    assert torch.equal(dres.view(torch.int16), want.view(torch.int16))
    dx2, none = ext().bn_bwd_dx(x, dy, y_arg, mean, invstd, gamma, dgamma,
                                dbeta, m_total, False, mask, asc, ash)
    assert none is None or none.numel() == 0
    assert torch.equal(dx2.view(torch.int16), dx.view(torch.int16))


@pytest.mark.parametrize("m_factor", [1, 2])         # 2: SyncBN, two ranks
@pytest.mark.parametrize("variant", ["none", "mask", "recompute"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", FAST_C)
def test_bn_bwd_dx_fast(C, dtype, variant, m_factor):
    for M in MS:
        _check_dx(C, M, dtype, variant, m_factor)


@pytest.mark.parametrize("m_factor", [1, 2])
@pytest.mark.parametrize("variant", ["none", "y"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", SLOW_C)
def test_bn_bwd_dx_fallback(C, dtype, variant, m_factor):
    for M in MS:
        _check_dx(C, M, dtype, variant, m_factor)


def test_bn_bwd_dx_grid_stride_boundary():
    C, M = BOUNDARY[0]
    _check_dx(C, M, torch.bfloat16, "mask", 1)


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("with_res", [False, True])
def test_batch_norm_constant_channel_end_to_end(with_res):
    """A constant channel (100.5 over 5000 rows) through fn.batch_norm in
    training mode: finite output and running stats, y = beta (+ res) on that
    channel, finite dx."""
    C, dtype = 8, torch.bfloat16
    g = torch.Generator().manual_seed(17)
    x = (torch.randn(5, 25, 40, C, generator=g) * 2 + 0.5)
    x[..., 0] = 100.5
    x = x.to(dtype).cuda().requires_grad_(True)
    res = (torch.randn(5, 25, 40, C, generator=g).to(dtype).cuda()
           if with_res else None)
    gamma = (torch.rand(C, generator=g) + 0.5).cuda().requires_grad_(True)
    beta = (torch.randn(C, generator=g) * 0.1).cuda().requires_grad_(True)
    rm, rv = torch.zeros(C).cuda(), torch.ones(C).cuda()
    y = fn.batch_norm(x, gamma, beta, rm, rv, True, 0.1, res, None)
    assert bool(torch.isfinite(y).all())
    assert bool(torch.isfinite(rm).all()) and bool(torch.isfinite(rv).all())
    assert bool((rv >= 0).all())
    # channel 0: x - mean is at most 3 * 2^-24 * 100.5 (the bound on the
    # kernel's mean), times gamma/sqrt(eps); the float64 value is beta (+res)
    ref = beta[0].detach().to(F64).expand(5, 25, 40)
    mag = beta[0].detach().to(F64).abs().expand(5, 25, 40)
    sc = gamma[0].detach().to(F64).abs() * EPS ** -0.5
    mag = mag + 2 * 100.5 * sc
    if with_res:
        ref = ref + res[..., 0].to(F64)
        mag = mag + res[..., 0].to(F64).abs()
    _assert_within(y.detach()[..., 0], ref, bn_apply_bound(ref, mag, dtype), "y[...,0]")
    dy = torch.randn(5, 25, 40, C, generator=g).to(dtype).cuda()
    y.backward(dy)
    assert bool(torch.isfinite(x.grad).all())
    assert bool(torch.isfinite(gamma.grad).all())
    assert bool(torch.isfinite(beta.grad).all())
