"""The whole-row epilogue store of the MFMA conv kernels (conv_epilogue.h)
through conv2d_fwd, conv2d_fwd_stats and conv2d_dgrad: exact element
placement with one-hot weights for every kernel family and tile width, the
residual add (exact, and rounded once), bias + ReLU, the BN statistics, and
random inputs against the fp32 CPU reference."""

import pytest
import torch
import torch.nn.functional as F

import mi355x.ops as ops
from mi355x.ops import functional as fn

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]


def _out(h, r, stride, pad):
    return (h + 2 * pad - r) // stride + 1


def _ints(shape, seed, lo=-8, hi=8):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _fwd(x, w, dtype, stride, pad, bias=None, act=0):
    """x: fp32 CPU NHWC, w: fp32 CPU [K,C,R,S] -> CPU fp32 y (NHWC)."""
    wg = w.cuda()
    w16 = fn._w16_conv(wg, dtype)
    b = (bias.cuda() if bias is not None
         else torch.empty(0, device="cuda", dtype=torch.float32))
    y = ops.ext().conv2d_fwd(x.cuda().to(dtype), w16, b, stride, pad, act,
                             w.shape[2], w.shape[3])
    assert y.dtype == dtype
    return y.float().cpu()


def _dgrad(dy, w, dtype, stride, pad, H, W, addin=None):
    """dy: fp32 CPU NHWC, w: fp32 CPU [K,C,R,S] -> CPU fp32 dx (NHWC)."""
    wf = fn._w16_conv_flip(w.cuda(), dtype)
    a = (addin.cuda().to(dtype) if addin is not None
         else torch.empty(0, device="cuda", dtype=dtype))
    dx = ops.ext().conv2d_dgrad(dy.cuda().to(dtype).contiguous(), wf, stride,
                                pad, H, W, a)
    assert dx.dtype == dtype
    return dx.float().cpu()


# ---- one-hot weights and the index-built expectations --------------------

def _taps(n_out, n_in, R):
    """For each output channel j: (input channel, r, s), all varying with j."""
    j = torch.arange(n_out)
    return (5 * j + 3) % n_in, (j // 2) % R, (j // 3 + j) % R


def _onehot_fwd(K, C, R):
    c, r, s = _taps(K, C, R)
    w = torch.zeros(K, C, R, R)
    w[torch.arange(K), c, r, s] = 1.0
    return w, (c, r, s)


def _onehot_dgrad(K, C, R):
    """w[k,c,r,s]: for each dx channel c one 1.0 at (k_c, r_c, s_c)."""
    k, r, s = _taps(C, K, R)
    w = torch.zeros(K, C, R, R)
    w[k, torch.arange(C), r, s] = 1.0
    return w, (k, r, s)


def _expect_fwd(x, taps, K, R, stride, pad):
    N, H, W, _ = x.shape
    P, Q = _out(H, R, stride, pad), _out(W, R, stride, pad)
    xp = F.pad(x, (0, 0, pad, pad, pad, pad))
    y = torch.zeros(N, P, Q, K)
    c, r, s = taps
    for k in range(K):
        rk, sk = int(r[k]), int(s[k])
        y[..., k] = xp[:, rk:rk + stride * (P - 1) + 1:stride,
                       sk:sk + stride * (Q - 1) + 1:stride, int(c[k])]
    return y


def _expect_dgrad(dy, taps, C, R, stride, pad, H, W):
    N, P, Q, _ = dy.shape
    k, r, s = taps
    dx = torch.zeros(N, H, W, C)
    Hp = max(R + stride * (P - 1) + 1, pad + H)
    Wp = max(R + stride * (Q - 1) + 1, pad + W)
    for c in range(C):
        rc, sc = int(r[c]), int(s[c])
        tmp = torch.zeros(N, Hp, Wp)
        tmp[:, rc:rc + stride * (P - 1) + 1:stride,
            sc:sc + stride * (Q - 1) + 1:stride] = dy[..., int(k[c])]
        dx[..., c] = tmp[:, pad:pad + H, pad:pad + W]
    return dx


def _same(got, want):
    assert got.shape == want.shape
    bad = (got != want).nonzero()
    assert bad.numel() == 0, (
        f"{bad.shape[0]} of {got.numel()} wrong, first at {bad[0].tolist()}: "
        f"{got[tuple(bad[0])].item()} != {want[tuple(bad[0])].item()}")


# name: (N, H, W, C, K, R, stride, pad)
PLACE = {
    # 3x3/s1: the patch kernel
    "p3_tile_and_half": (3, 8, 8, 64, 64, 3, 1, 1),    # M = 192
    "p3_m32_3kblocks": (2, 4, 4, 128, 192, 3, 1, 1),   # M = 32 < 128
    "p3_odd_w": (5, 7, 7, 64, 128, 3, 1, 1),           # tiles cross images
    # 1x1 and stride 2: the gather kernel (fwd), the parity kernel (dgrad)
    "g1_s1": (3, 8, 8, 64, 128, 1, 1, 0),
    "g1_s2": (3, 8, 8, 64, 128, 1, 2, 0),
    "g3_s2_even": (3, 8, 8, 64, 128, 3, 2, 1),
    "g3_s2_odd": (3, 7, 7, 64, 128, 3, 2, 1),          # unequal parity classes
}
# the 128-channel-wide tiles are only chosen for M >= 128 * 1024 (gather) or
# a parity class of >= 128 * 256 rows with 128 dx channels (stride-2 dgrad)
PLACE_WIDE_FWD = {"g1_s1_wide": (32, 64, 64, 64, 128, 1, 1, 0)}
PLACE_WIDE_DGRAD = {
    "g1_s1_wide": (32, 64, 64, 128, 64, 1, 1, 0),
    "g1_s2_wide": (32, 64, 64, 128, 64, 1, 2, 0),
}


def _place_fwd(case, dtype, bias=None, act=0):
    N, H, W, C, K, R, stride, pad = case
    x = _ints((N, H, W, C), seed=H * W + C)
    w, taps = _onehot_fwd(K, C, R)
    want = _expect_fwd(x, taps, K, R, stride, pad)
    if bias is not None:
        want = want + bias
    if act == 1:
        want = want.clamp_min(0)
    _same(_fwd(x, w, dtype, stride, pad, bias, act), want)


def _place_dgrad(case, dtype, with_addin):
    N, H, W, C, K, R, stride, pad = case
    P, Q = _out(H, R, stride, pad), _out(W, R, stride, pad)
    dy = _ints((N, P, Q, K), seed=P * Q + K)
    w, taps = _onehot_dgrad(K, C, R)
    want = _expect_dgrad(dy, taps, C, R, stride, pad, H, W)
    addin = None
    if with_addin:
        addin = _ints((N, H, W, C), seed=7 * H + C)  # |sum| <= 16: exact
        want = want + addin
    _same(_dgrad(dy, w, dtype, stride, pad, H, W, addin), want)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", list(PLACE))
def test_fwd_placement(name, dtype):
    _place_fwd(PLACE[name], dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", list(PLACE))
def test_dgrad_placement(name, dtype):
    _place_dgrad(PLACE[name], dtype, with_addin=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", list(PLACE))
def test_dgrad_addin_exact(name, dtype):
    _place_dgrad(PLACE[name], dtype, with_addin=True)


@pytest.mark.parametrize("name", list(PLACE_WIDE_FWD))
def test_fwd_placement_wide(name):
    _place_fwd(PLACE_WIDE_FWD[name], torch.bfloat16)


@pytest.mark.parametrize("with_addin", [False, True], ids=["plain", "addin"])
@pytest.mark.parametrize("name", list(PLACE_WIDE_DGRAD))
def test_dgrad_placement_wide(name, with_addin):
    _place_dgrad(PLACE_WIDE_DGRAD[name], torch.bfloat16, with_addin)


# the C=3 stems: strip kernel (Ho*Wo % 128 == 0) and its gather fallback
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("hw", [32, 30], ids=["strip", "fallback"])
def test_stem_fwd_placement(hw, dtype):
    _place_fwd((2, hw, hw, 3, 64, 3, 1, 1), dtype)


# a channel count that is no multiple of 64: the per-element gather variant
def test_genc_fwd_placement():
    _place_fwd((2, 10, 10, 24, 64, 3, 1, 1), torch.bfloat16)


# ---- ADDIN is added in fp32 and the sum rounded once ---------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_addin_rounded_once(dtype):
    # ulp(1.0) is 2^-7 in bf16 and 2^-10 in fp16. acc = 1 + ulp/4 is exact
    # in fp32; adding ulp/2 gives 1 + 0.75 ulp -> 1 + ulp. Rounding acc
    # first gives 1.0, then 1 + ulp/2 ties to even: 1.0.
    ulp = 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -10
    N, H, W, C, K = 3, 8, 8, 64, 128
    dy = torch.empty(N, H, W, K)
    dy[..., :64] = 1.0
    dy[..., 64:] = ulp / 4
    w = torch.zeros(K, C, 3, 3)
    c = torch.arange(C)
    w[c, c, 1, 1] = 1.0        # two-hot: dx[c] = dy[c] + dy[64 + c]
    w[64 + c, c, 1, 1] = 1.0
    addin = torch.full((N, H, W, C), ulp / 2)
    acc = F.conv_transpose2d(dy.permute(0, 3, 1, 2), w,
                             padding=1).permute(0, 2, 3, 1)
    want = (acc + addin).to(dtype).float()
    twice = (acc.to(dtype).float() + addin).to(dtype).float()
    assert (want == 1.0 + ulp).all() and (twice == 1.0).all()
    _same(_dgrad(dy, w, dtype, 1, 1, H, W, addin), want)


# ---- bias + ReLU ----------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("act", [0, 1], ids=["linear", "relu"])
def test_bias_relu_exact(act, dtype):
    bias = _ints((64,), seed=9, lo=-4, hi=4)
    _place_fwd(PLACE["p3_tile_and_half"], dtype, bias=bias, act=act)


# ---- random data: fwd, stats, dgrad, dgrad + ADDIN -----------------------

RTOL, ATOL = 3e-2, 3e-2  # the conv tolerances of test_gpu_kernels.py


def _rand_case(N, H, W, C, K, seed):
    g = torch.Generator().manual_seed(seed)
    q = lambda t: t.to(torch.bfloat16).float()
    x = q(torch.randn(N, H, W, C, generator=g))
    w = q(torch.randn(K, C, 3, 3, generator=g) * 0.1)
    dy = q(torch.randn(N, H, W, K, generator=g))
    addin = q(torch.randn(N, H, W, C, generator=g))
    y = F.conv2d(x.permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1)
    dx = F.conv_transpose2d(dy.permute(0, 3, 1, 2), w,
                            padding=1).permute(0, 2, 3, 1)
    return dict(x=x, w=w, dy=dy, addin=addin, y=y.contiguous(),
                dx=dx.contiguous())


RAND_SHAPES = {"c64": (3, 8, 8, 64, 64), "c128": (5, 7, 7, 64, 128),
               "c256": (2, 4, 4, 256, 256)}


@pytest.fixture(scope="module")
def rand_ref():
    return {k: _rand_case(*v, seed=len(k)) for k, v in RAND_SHAPES.items()}


@pytest.mark.parametrize("name", ["c64", "c256"])
def test_random_vs_cpu(name, rand_ref):
    r = rand_ref[name]
    N, H, W, C, K = RAND_SHAPES[name]
    bf = torch.bfloat16
    torch.testing.assert_close(_fwd(r["x"], r["w"], bf, 1, 1), r["y"],
                               rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(_dgrad(r["dy"], r["w"], bf, 1, 1, H, W),
                               r["dx"], rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(
        _dgrad(r["dy"], r["w"], bf, 1, 1, H, W, r["addin"]),
        r["dx"] + r["addin"], rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("name", ["c64", "c128"])
def test_stats(name, rand_ref):
    r = rand_ref[name]
    K = RAND_SHAPES[name][4]
    x = r["x"].cuda().to(torch.bfloat16)
    w16 = fn._w16_conv(r["w"].cuda(), torch.bfloat16)
    e = torch.empty(0, device="cuda", dtype=torch.float32)
    y0 = ops.ext().conv2d_fwd(x, w16, e, 1, 1, 0, 3, 3)
    y1, s1 = ops.ext().conv2d_fwd_stats(x, w16, 1, 1, 3, 3)
    y2, s2 = ops.ext().conv2d_fwd_stats(x, w16, 1, 1, 3, 3)
    assert torch.equal(y1, y0) and torch.equal(y2, y0)
    assert s1.shape == (2, K) and torch.equal(s1, s2)
    yf = r["y"].reshape(-1, K)
    ref = torch.stack([yf.sum(0), (yf * yf).sum(0)])
    err = (s1.cpu() - ref).abs().max().item()
    print(f"{name}: max |stats - ref| {err:.3e}")
    # the tolerance of test_conv_bn_fused_stats_matches_separate
    torch.testing.assert_close(s1.cpu(), ref, rtol=2e-2, atol=2.0)
