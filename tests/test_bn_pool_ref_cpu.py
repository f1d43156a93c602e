"""The float64 references of _bn_pool_ref.py against torch's own float64
batch_norm / max_pool2d / mean with autograd, on tie-free random inputs, and
the first-index tie rule on a hand-written case: the references are proven
here before they judge a kernel."""

import pytest
import torch
import torch.nn.functional as F

from _bn_pool_ref import (bn_apply_ref, bn_bwd_ref, bn_finalize_ref,
                          fp32_sum_bound, gap_bwd_ref, gap_ref, maxpool_bwd_ref,
                          maxpool_ref, pool_out, u16)

F64 = torch.float64
EPS = 1e-5
# float64 against float64: both sides round ~1e-16 per operation; the
# variance (sumsq/m - mean^2) cancels a few digits
TOL = dict(rtol=1e-10, atol=1e-11)


def _bn_inputs(M, C, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, C, generator=g) * 2 + 0.5).to(dtype)
    res = torch.randn(M, C, generator=g).to(dtype)
    dy = torch.randn(M, C, generator=g).to(dtype)
    gamma = torch.rand(C, generator=g) + 0.5
    gamma[0] = -0.75
    beta = torch.randn(C, generator=g) * 0.1
    rm = torch.randn(C, generator=g)
    rv = torch.rand(C, generator=g) + 0.5
    return x, res, dy, gamma, beta, rm, rv


def _stats(x):
    xd = x.to(F64)
    return torch.stack([xd.sum(0), (xd * xd).sum(0)])


def test_bounds_helpers():
    assert u16(torch.bfloat16) == 2.0 ** -8
    assert u16(torch.float16) == 2.0 ** -11
    with pytest.raises(ValueError):
        u16(torch.float32)
    t = torch.tensor([[1.0, -2.0], [-3.0, 4.0]], dtype=F64)
    assert torch.equal(fp32_sum_bound(2, t),
                       6 * 2.0 ** -24 * torch.tensor([4.0, 6.0], dtype=F64))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M,momentum", [(37, 0.1), (2, 1.0), (700, 0.1)])
def test_bn_forward_refs_match_torch(dtype, M, momentum):
    C = 6
    x, res, _, gamma, beta, rm, rv = _bn_inputs(M, C, dtype)
    rm_t, rv_t = rm.to(F64), rv.to(F64)
    out, save_mean, save_invstd = torch.native_batch_norm(
        x.to(F64), gamma.to(F64), beta.to(F64), rm_t, rv_t, True, momentum,
        EPS)
    fin = bn_finalize_ref(_stats(x), rm, rv, M, momentum, EPS)
    torch.testing.assert_close(fin.mean, save_mean, **TOL)
    torch.testing.assert_close(fin.invstd, save_invstd, **TOL)
    torch.testing.assert_close(fin.running_mean, rm_t, **TOL)
    torch.testing.assert_close(fin.running_var, rv_t, **TOL)
    assert bool((fin.dvar > 0).all())

    y, mag = bn_apply_ref(x, fin.mean, fin.invstd, gamma, beta, None, False)
    torch.testing.assert_close(y, out, **TOL)
    assert bool((mag >= y.abs() * (1 - 1e-12)).all())
    y, _ = bn_apply_ref(x, fin.mean, fin.invstd, gamma, beta, res, True)
    torch.testing.assert_close(y, F.relu(out + res.to(F64)), **TOL)
    # an empty residual is "none", as the kernels take it
    y2, _ = bn_apply_ref(x, fin.mean, fin.invstd, gamma, beta,
                         torch.empty(0, dtype=dtype), True)
    torch.testing.assert_close(y2, F.relu(out), **TOL)


def test_bn_finalize_ref_edges():
    # m = 1: unbias factor 1, variance 0; no running stats: none returned
    s = torch.tensor([[3.0], [9.0]])
    fin = bn_finalize_ref(s, torch.zeros(1), torch.zeros(1), 1, 1.0, EPS)
    assert fin.var.item() == 0.0 and fin.running_var.item() == 0.0
    assert fin.invstd.item() == pytest.approx(EPS ** -0.5, rel=1e-14)
    fin = bn_finalize_ref(s, torch.empty(0), torch.empty(0), 1, 0.1, EPS)
    assert fin.running_mean is None and fin.running_var is None
    # inconsistent (rounded) sums of a constant channel: clamped at 0
    s = torch.tensor([[100.5 * 5000], [100.5 ** 2 * 5000 - 4]])
    fin = bn_finalize_ref(s, torch.zeros(1), torch.zeros(1), 5000, 0.1, EPS)
    assert fin.var.item() == 0.0 and fin.running_var.item() == 0.0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("relu", [False, True])
def test_bn_bwd_ref_matches_autograd(dtype, relu):
    M, C = 61, 6
    x, res, dy, gamma, beta, _, _ = _bn_inputs(M, C, dtype, seed=1)
    xa = x.to(F64).requires_grad_(True)
    ga = gamma.to(F64).requires_grad_(True)
    ba = beta.to(F64).requires_grad_(True)
    ra = res.to(F64).requires_grad_(True)
    y = F.batch_norm(xa, None, None, ga, ba, True, 0.1, EPS) + ra
    if relu:
        y = F.relu(y)
    y.backward(dy.to(F64))
    keep = (y.detach() > 0) if relu else None

    fin = bn_finalize_ref(_stats(x), None, None, M, 0.1, EPS)
    r = bn_bwd_ref(x, dy, keep, fin.mean, fin.invstd, gamma, None, None, M)
    assert r.dx is None
    dgamma, dbeta = r.t_dgamma.sum(0), r.t_dbeta.sum(0)
    torch.testing.assert_close(dgamma, ga.grad, **TOL)
    torch.testing.assert_close(dbeta, ba.grad, **TOL)
    torch.testing.assert_close(r.d, ra.grad, **TOL)
    r = bn_bwd_ref(x, dy, keep, fin.mean, fin.invstd, gamma, dgamma, dbeta, M)
    torch.testing.assert_close(r.dx, xa.grad, **TOL)
    assert bool((r.mag >= r.dx.abs() * (1 - 1e-12)).all())


def test_bn_bwd_ref_m_total_is_the_global_batch():
    """SyncBN: each rank holds half the rows; stats and (dgamma, dbeta) are
    global, m_total = 2M. The per-rank reference dx must be the matching
    half of the full-batch autograd gradient."""
    M, C = 40, 6
    x, _, dy, gamma, beta, _, _ = _bn_inputs(2 * M, C, torch.bfloat16, seed=2)
    xa = x.to(F64).requires_grad_(True)
    y = F.batch_norm(xa, None, None, gamma.to(F64), beta.to(F64), True, 0.1,
                     EPS)
    y.backward(dy.to(F64))
    fin = bn_finalize_ref(_stats(x), None, None, 2 * M, 0.1, EPS)
    full = bn_bwd_ref(x, dy, None, fin.mean, fin.invstd, gamma, None, None,
                      2 * M)
    dgamma, dbeta = full.t_dgamma.sum(0), full.t_dbeta.sum(0)
    for half in (slice(0, M), slice(M, 2 * M)):
        r = bn_bwd_ref(x[half], dy[half], None, fin.mean, fin.invstd, gamma,
                       dgamma, dbeta, 2 * M)
        torch.testing.assert_close(r.dx, xa.grad[half], **TOL)


GEOMS = [(2, 2, 0), (3, 2, 1), (3, 1, 1), (3, 3, 0), (2, 3, 0), (5, 2, 2)]
SIZES = [(7, 9), (8, 8), (10, 6)]


def _tie_free(N, H, W, C, dtype, seed):
    """Every (n, c) plane is a permutation of H*W distinct small integers:
    exact in both 16-bit types, and no window holds a tie."""
    g = torch.Generator().manual_seed(seed)
    planes = torch.stack([torch.randperm(H * W, generator=g)
                          for _ in range(N * C)]).float() - (H * W) // 2
    return planes.reshape(N, C, H, W).permute(0, 2, 3, 1).contiguous().to(dtype)


def _torch_rel_idx(ind, P, Q, W, s, p, k):
    """torch's absolute ih*W + iw (NCHW) -> relative r*k + c (NHWC)."""
    ih, iw = ind // W, ind % W
    pi = torch.arange(P).reshape(1, 1, P, 1)
    qi = torch.arange(Q).reshape(1, 1, 1, Q)
    rel = (ih - (pi * s - p)) * k + (iw - (qi * s - p))
    return rel.permute(0, 2, 3, 1).to(torch.uint8)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("k,s,p", GEOMS)
def test_maxpool_refs_match_torch(dtype, k, s, p):
    N, C = 3, 6
    for H, W in SIZES:
        x = _tie_free(N, H, W, C, dtype, seed=H * W + k)
        xa = x.to(F64).permute(0, 3, 1, 2).requires_grad_(True)
        yt, ind = F.max_pool2d(xa, k, s, p, return_indices=True)
        P, Q = pool_out(H, k, s, p), pool_out(W, k, s, p)
        assert yt.shape == (N, C, P, Q)
        y, idx = maxpool_ref(x, k, s, p)
        assert y.dtype == dtype and idx.dtype == torch.uint8
        assert torch.equal(y.to(F64), yt.detach().permute(0, 2, 3, 1))
        assert torch.equal(idx, _torch_rel_idx(ind, P, Q, W, s, p, k))
        # float32 work type: same answer (a max of 16-bit values is exact)
        y32, idx32 = maxpool_ref(x, k, s, p, work=torch.float32)
        assert torch.equal(y32, y) and torch.equal(idx32, idx)

        g = torch.Generator().manual_seed(7)
        dy = torch.randn(N, P, Q, C, generator=g).to(dtype)
        yt.backward(dy.to(F64).permute(0, 3, 1, 2))
        b = maxpool_bwd_ref(dy, idx, H, W, k, s, p)
        torch.testing.assert_close(b.dx, xa.grad.permute(0, 2, 3, 1), **TOL)
        assert int(b.count.sum()) == dy.numel()
        assert int(b.count.max()) <= ((k + s - 1) // s) ** 2
        assert bool((b.abs_sum >= b.dx.abs() * (1 - 1e-12)).all())


def test_maxpool_ref_first_index_tie_rule():
    # one 4x4 plane, 3x3/s2/p1 -> 2x2 windows
    plane = torch.tensor([[1., 5., 5., 0.],
                          [5., 5., 2., 2.],
                          [3., 3., 7., 7.],
                          [3., 3., 7., 7.]])
    x = plane.reshape(1, 4, 4, 1).to(torch.bfloat16)
    y, idx = maxpool_ref(x, 3, 2, 1)
    assert y.reshape(2, 2).tolist() == [[5., 5.], [5., 7.]]
    # window (0,0) covers rows/cols -1..1: in-image taps (1,1)=1, (1,2)=5,
    # (2,1)=5, (2,2)=5 -> first max at tap (1,2) = 5. Window (0,1): cols
    # 1..3, taps (1,0)=5 first. Window (1,0): rows 1..3, cols -1..1: (0,1)=5
    # first. Window (1,1): rows 1..3, cols 1..3: first 7 at tap (1,1).
    assert idx.reshape(2, 2).tolist() == [[5, 3], [1, 4]]
    dy = torch.tensor([[1., 2.], [4., 8.]]).reshape(1, 2, 2, 1)
    b = maxpool_bwd_ref(dy.to(torch.bfloat16), idx, 4, 4, 3, 2, 1)
    want = torch.zeros(4, 4, dtype=F64)
    want[0, 1] = 1 + 2     # both top windows picked pixel (0,1)
    want[1, 0] = 4
    want[2, 2] = 8
    assert torch.equal(b.dx.reshape(4, 4), want)
    assert b.count.reshape(4, 4)[0, 1] == 2
    assert b.abs_sum.reshape(4, 4)[0, 1] == 3


def test_maxpool_ref_nonfinite_as_torch():
    """NaN beats everything and padding never wins, as in torch."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 8, 8, 3, generator=g).to(torch.bfloat16)
    x[0, 3, 4, 1] = float("nan")
    x[1, 0, 0, 0] = float("nan")
    x[0, 0:3, 0:3, 2] = float("-inf")    # window (0,0) of 3/2/1: all -inf
    x[1, 5, 5, 2] = float("inf")
    xa = x.to(F64).permute(0, 3, 1, 2)
    yt, ind = F.max_pool2d(xa, 3, 2, 1, return_indices=True)
    y, idx = maxpool_ref(x, 3, 2, 1)
    yt = yt.permute(0, 2, 3, 1)
    assert torch.equal(torch.isnan(y), torch.isnan(yt))
    assert int(torch.isnan(y).sum()) == 2 + 1   # pixel (3,4): 2 windows
    ok = ~torch.isnan(yt)
    assert torch.equal(y.to(F64)[ok], yt[ok])
    assert y[0, 0, 0, 2] == float("-inf") and bool((y == float("inf")).any())
    assert torch.equal(idx, _torch_rel_idx(ind, 4, 4, 8, 2, 1, 3))
    with pytest.raises(ValueError):
        maxpool_ref(x, 3, 2, 2)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_gap_refs_match_torch(dtype):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 7, 7, 10, generator=g).to(dtype)
    xa = x.to(F64).requires_grad_(True)
    yt = xa.mean(dim=(1, 2))
    y, absmean = gap_ref(x)
    torch.testing.assert_close(y, yt, **TOL)
    assert bool((absmean >= y.abs() * (1 - 1e-12)).all())
    dy = torch.randn(2, 10, generator=g).to(dtype)
    yt.backward(dy.to(F64))
    torch.testing.assert_close(gap_bwd_ref(dy, 7, 7), xa.grad, **TOL)
