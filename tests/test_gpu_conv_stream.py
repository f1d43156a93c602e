"""The streaming patch kernel of the 128/256/512-channel 3x3/s1 layers
(conv_patch_stream: a persistent block keeps one 64-channel output tile and
walks 256-output m-tiles as one flat sequence of (m-tile, c-chunk) stages)
through conv2d_fwd, conv2d_fwd_stats and conv2d_dgrad: exact placement with
one-hot weights and with impulses at every tile, image, pad-column and
M-tail edge, exact BN statistics, the same bits as conv_patch_gemm, random
inputs against the fp32 CPU reference, and the routing predicate.

Knobs are read once per process, so the runs that need one (the old kernel,
MI355X_PATCH_STREAM=0; several m-tiles per block,
MI355X_PATCH_STREAM_BLOCKS=2) happen in two child processes, one per knob,
shared by the tests."""

import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import mi355x.ops as ops
from mi355x.ops import functional as fn
from tests.test_gpu_conv_epilogue import (_dgrad, _expect_dgrad, _expect_fwd,
                                          _fwd, _ints, _onehot_dgrad,
                                          _onehot_fwd, _same)

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}

# name: (N, H, W, CI, KO). CI is the channel count of the tensor the kernel
# reads (x in fwd, dy in dgrad), KO that of the one it writes. A tile is 256
# outputs, a half 128.
SHAPES = {
    "one_tile": (1, 16, 16, 128, 64),      # two c-chunks, both halos outside
    "three_tiles": (3, 16, 16, 128, 64),   # hand-over; 2 blocks: runs 2 and 1
    "half_empty": (3, 8, 8, 128, 64),      # M = 192: second half half empty
    "two_k_tiles": (5, 4, 4, 128, 128),    # M = 80: images cross, partial
    "w4_tail": (40, 4, 4, 128, 64),        # M = 640: 2.5 tiles, 16 images each
    "four_chunks": (2, 8, 8, 256, 64),
    "h_not_w": (2, 6, 8, 128, 64),         # M = 96
}
# the routing predicate: these stay on conv_patch_gemm (widths whose tiles
# would start mid-row, the 64-channel layer, and every SCALED call)
NOT_ELIGIBLE = {
    "w7": (2, 7, 7, 128, 64),
    "w14": (2, 14, 14, 128, 64),
    "ci64_w32": (2, 8, 32, 64, 64),
}


# ---- running the ops, here or in a child process -------------------------

def _run_ops(jobs):
    """jobs: {key: (op, dtype name, tensors...)}, fp32 CPU tensors in NHWC
    and [K,C,3,3] -> {key: fp32 CPU result}."""
    out = {}
    for key, (op, dt, *t) in jobs.items():
        dtype = DT[dt]
        if op == "fwd":
            out[key] = _fwd(t[0], t[1], dtype, 1, 1)
        elif op == "stats":
            w16 = fn._w16_conv(t[1].cuda(), dtype)
            y, s = ops.ext().conv2d_fwd_stats(t[0].cuda().to(dtype), w16,
                                              1, 1, 3, 3)
            out[key] = (y.float().cpu(), s.cpu())
        elif op == "scaled":
            w16 = fn._w16_conv(t[1].cuda(), dtype)
            y = ops.ext().conv2d_fwd_scaled(t[0].cuda().to(dtype), w16,
                                            t[2].cuda(), t[3].cuda(), 1, 1,
                                            False)[0]
            out[key] = y.float().cpu()
        else:
            H, W = t[0].shape[1:3]
            out[key] = _dgrad(t[0], t[1], dtype, 1, 1, H, W,
                              t[2] if len(t) > 2 else None)
    return out


CHILD = """
import sys, torch
from tests.test_gpu_conv_stream import _run_ops
torch.save(_run_ops(torch.load(sys.argv[1])), sys.argv[2])
"""


def _run_child(jobs, tmp, **knobs):
    inp, out = str(tmp / "jobs.pt"), str(tmp / "results.pt")
    torch.save(jobs, inp)
    r = subprocess.run([sys.executable, "-c", CHILD, inp, out], cwd=REPO,
                       env=dict(os.environ, **knobs), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + "\n" + r.stderr[-2500:]
    return torch.load(out)


# ---- the cases: inputs (jobs) and what must come out (wants) -------------

def _place_case(key, shape, dt):
    """One-hot weights, small-integer inputs: fwd, dgrad, dgrad + ADDIN."""
    N, H, W, CI, KO = shape
    a = _ints((N, H, W, CI), seed=H * W + KO + N)
    wf, tf = _onehot_fwd(KO, CI, 3)
    wd, td = _onehot_dgrad(CI, KO, 3)  # dy has the CI channels, dx the KO
    addin = _ints((N, H, W, KO), seed=7 * H + KO)  # |sum| <= 16: exact
    dx = _expect_dgrad(a, td, KO, 3, 1, 1, H, W)
    jobs = {f"{key}-fwd": ("fwd", dt, a, wf),
            f"{key}-dgrad": ("dgrad", dt, a, wd),
            f"{key}-addin": ("dgrad", dt, a, wd, addin)}
    wants = {f"{key}-fwd": _expect_fwd(a, tf, KO, 3, 1, 1),
             f"{key}-dgrad": dx, f"{key}-addin": dx + addin}
    return jobs, wants


# M = 320: tile 0 is images 0-3 (halves change at image 2), tile 1 is image 4
# alone, a quarter tile. With two blocks each runs one of them.
IMP_SHAPE = (5, 8, 8, 128, 64)
# name: [(n, p, q), ...] of the 1.0s
IMPULSES = {
    "tile_first_pixel": [(4, 0, 0)],
    "tile_last_pixel": [(3, 7, 7)],
    "half_change": [(1, 7, 7), (2, 0, 0)],
    "image_first_row": [(1, 0, 5)],
    "image_last_row": [(1, 7, 2)],
    "pad_column_left": [(0, 2, 0)],
    "pad_column_right": [(0, 5, 7)],
    "image_change": [(0, 7, 3), (1, 0, 3), (3, 7, 4)],
    "last_row_before_tail": [(4, 7, 1), (4, 7, 7)],
}


def _impulse_case(name):
    """Impulse input, dense small-integer weights: every product and sum is
    a small integer, so F.conv2d in fp32 on the CPU is the exact answer."""
    N, H, W, CI, KO = IMP_SHAPE
    i = list(IMPULSES).index(name)
    a = torch.zeros(N, H, W, CI)
    for j, (n, p, q) in enumerate(IMPULSES[name]):
        a[n, p, q, (7 * i + 3 + 71 * j) % CI] = 1.0
    w = _ints((KO, CI, 3, 3), seed=40 + i, lo=-3, hi=3)
    addin = _ints((N, H, W, KO), seed=60 + i)
    an = a.permute(0, 3, 1, 2)
    y = F.conv2d(an, w, padding=1).permute(0, 2, 3, 1).contiguous()
    wt = _ints((CI, KO, 3, 3), seed=80 + i, lo=-3, hi=3)  # dgrad: [K=CI, C=KO]
    dx = F.conv_transpose2d(an, wt, padding=1).permute(0, 2, 3, 1).contiguous()
    jobs = {f"imp-{name}-fwd": ("fwd", "bf16", a, w),
            f"imp-{name}-dgrad": ("dgrad", "bf16", a, wt),
            f"imp-{name}-addin": ("dgrad", "bf16", a, wt, addin)}
    wants = {f"imp-{name}-fwd": y, f"imp-{name}-dgrad": dx,
             f"imp-{name}-addin": dx + addin}
    return jobs, wants


def _once_case(dt):
    """ADDIN is added in fp32 and the sum rounded once (the check of
    test_gpu_conv_epilogue.test_addin_rounded_once, at 128 dy channels):
    acc = 1 + ulp/4 is exact in fp32; adding ulp/2 gives 1 + 0.75 ulp ->
    1 + ulp. Rounding acc first gives 1.0, then 1 + ulp/2 ties to 1.0."""
    ulp = 2.0 ** -7 if dt == "bf16" else 2.0 ** -10
    N, H, W, CI, KO = SHAPES["three_tiles"]
    dy = torch.zeros(N, H, W, CI)
    dy[..., :32] = 1.0
    dy[..., 32:64] = ulp / 4
    w = torch.zeros(CI, KO, 3, 3)
    c = torch.arange(KO)
    w[c % 32, c, 1, 1] = 1.0  # two-hot: dx[c] = dy[c % 32] + dy[32 + c % 32]
    w[32 + c % 32, c, 1, 1] = 1.0
    addin = torch.full((N, H, W, KO), ulp / 2)
    acc = F.conv_transpose2d(dy.permute(0, 3, 1, 2), w,
                             padding=1).permute(0, 2, 3, 1)
    want = (acc + addin).to(DT[dt]).float()
    twice = (acc.to(DT[dt]).float() + addin).to(DT[dt]).float()
    assert (want == 1.0 + ulp).all() and (twice == 1.0).all()
    return {f"once-{dt}": ("dgrad", dt, dy, w, addin)}, {f"once-{dt}": want}


def _rand_case(name, dt):
    """Random inputs, rounded to the dtype; fp32 CPU references."""
    N, H, W, CI, KO = SHAPES[name]
    g = torch.Generator().manual_seed(len(name) + len(dt) * 100 + KO + N)
    q = lambda t: t.to(DT[dt]).float()
    a = q(torch.randn(N, H, W, CI, generator=g))
    wf = q(torch.randn(KO, CI, 3, 3, generator=g) * 0.1)
    wd = q(torch.randn(CI, KO, 3, 3, generator=g) * 0.1)
    addin = q(torch.randn(N, H, W, KO, generator=g))
    an = a.permute(0, 3, 1, 2)
    y = F.conv2d(an, wf, padding=1).permute(0, 2, 3, 1).contiguous()
    dx = F.conv_transpose2d(an, wd, padding=1).permute(0, 2, 3, 1).contiguous()
    key = f"rand-{name}-{dt}"
    jobs = {f"{key}-fwd": ("fwd", dt, a, wf),
            f"{key}-stats": ("stats", dt, a, wf),
            f"{key}-dgrad": ("dgrad", dt, a, wd),
            f"{key}-addin": ("dgrad", dt, a, wd, addin)}
    refs = {f"{key}-fwd": y, f"{key}-dgrad": dx, f"{key}-addin": dx + addin}
    return jobs, refs


def _merge(cases):
    jobs, wants = {}, {}
    for j, w in cases:
        jobs.update(j)
        wants.update(w)
    return jobs, wants


@pytest.fixture(scope="module")
def rand_cases():
    return _merge(_rand_case(n, dt) for n in SHAPES for dt in DT)


@pytest.fixture(scope="module")
def old_kernel(rand_cases, tmp_path_factory):
    """conv_patch_gemm on the random cases."""
    return _run_child(rand_cases[0], tmp_path_factory.mktemp("stream_off"),
                      MI355X_PATCH_STREAM="0")


@pytest.fixture(scope="module")
def two_blocks(rand_cases, tmp_path_factory):
    """Everything with two blocks (one per k-tile where there are two), so
    that a block runs several m-tiles and fetches the next tile's operands
    during the last c-chunk of the current one: (jobs' results, wants of the
    exact cases)."""
    jobs, wants = _merge(
        [_place_case(f"{n}-{dt}", s, dt) for n, s in SHAPES.items()
         for dt in DT] + [_impulse_case(n) for n in IMPULSES] +
        [_once_case(dt) for dt in DT])
    jobs.update(rand_cases[0])
    got = _run_child(jobs, tmp_path_factory.mktemp("stream_2blocks"),
                     MI355X_PATCH_STREAM_BLOCKS="2")
    return got, wants


@pytest.fixture(scope="module")
def stream_rand(rand_cases):
    """The streaming kernel on the random cases, a block per CU."""
    return _run_ops(rand_cases[0])


def _check(got, wants):
    assert wants
    for key, want in wants.items():
        _same(got[key], want)


# ---- 1. exact placement ----------------------------------------------------

@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("name", list(SHAPES))
def test_placement(name, dt):
    jobs, wants = _place_case(f"{name}-{dt}", SHAPES[name], dt)
    _check(_run_ops(jobs), wants)


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("name", list(SHAPES))
def test_placement_two_blocks(name, dt, two_blocks):
    got, wants = two_blocks
    _check(got, {k: v for k, v in wants.items()
                 if k.startswith(f"{name}-{dt}-")})


@pytest.mark.parametrize("name", list(IMPULSES))
def test_impulse(name):
    jobs, wants = _impulse_case(name)
    _check(_run_ops(jobs), wants)


@pytest.mark.parametrize("name", list(IMPULSES))
def test_impulse_two_blocks(name, two_blocks):
    got, wants = two_blocks
    _check(got, {k: v for k, v in wants.items()
                 if k.startswith(f"imp-{name}-")})


@pytest.mark.parametrize("dt", list(DT))
def test_addin_rounded_once(dt, two_blocks):
    jobs, wants = _once_case(dt)
    _check(_run_ops(jobs), wants)
    got, wants2 = two_blocks
    _same(got[f"once-{dt}"], wants2[f"once-{dt}"])


# ---- 2. BN statistics, exact ----------------------------------------------

@pytest.mark.parametrize("name", ["three_tiles", "two_k_tiles", "w4_tail"])
def test_stats_exact(name):
    """Integers of |y| <= 8 over at most 768 rows: every partial sum is an
    integer below 2^24, so fp32 sums are exact in any order."""
    N, H, W, CI, KO = SHAPES[name]
    x = _ints((N, H, W, CI), seed=H + N)
    w, taps = _onehot_fwd(KO, CI, 3)
    y, s = _run_ops({"s": ("stats", "bf16", x, w)})["s"]
    want = _expect_fwd(x, taps, KO, 3, 1, 1)
    _same(y, want)
    wf = want.reshape(-1, KO)
    _same(s, torch.stack([wf.sum(0), (wf * wf).sum(0)]))


# ---- 3. the same bits as conv_patch_gemm, and from call to call -----------

def _equal(a, b):
    if isinstance(a, tuple):
        return all(torch.equal(x, y) for x, y in zip(a, b))
    return torch.equal(a, b)


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("name", list(SHAPES))
def test_bit_identical_to_patch_gemm(name, dt, old_kernel, stream_rand,
                                     two_blocks):
    """Every output element is the same sequence of MFMAs (c-chunk, tap
    0..8, kk 0..3) and every stats row the same fold as in conv_patch_gemm,
    which a fresh process with MI355X_PATCH_STREAM=0 runs."""
    for op in ("fwd", "stats", "dgrad", "addin"):
        key = f"rand-{name}-{dt}-{op}"
        assert _equal(stream_rand[key], old_kernel[key]), key
        assert _equal(two_blocks[0][key], old_kernel[key]), key + " (2 blocks)"


def test_bit_repeatable(rand_cases, stream_rand):
    again = _run_ops(rand_cases[0])
    for key, got in stream_rand.items():
        assert _equal(again[key], got), key


# ---- 4. random inputs against the fp32 CPU reference ----------------------

@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("name", list(SHAPES))
def test_random_vs_cpu(name, dt, rand_cases, old_kernel, stream_rand):
    """max |out - fp32 CPU reference| of both kernels in the same run: the
    new kernel's may not exceed twice conv_patch_gemm's (being the same
    bits, it equals it; the figures are in profiles/r08_conv_stream.md)."""
    refs = rand_cases[1]
    for op in ("fwd", "dgrad", "addin"):
        key = f"rand-{name}-{dt}-{op}"
        err = lambda t: (t - refs[key]).abs().max().item()
        e_new, e_old = err(stream_rand[key]), err(old_kernel[key])
        print(f"{key}: max abs err {e_new:.4e}, conv_patch_gemm {e_old:.4e}")
        assert e_new <= 2 * e_old


# ---- 5. not eligible: stays on conv_patch_gemm ----------------------------

@pytest.mark.parametrize("name", list(NOT_ELIGIBLE))
def test_not_eligible_placement(name):
    jobs, wants = _place_case(name, NOT_ELIGIBLE[name], "bf16")
    _check(_run_ops(jobs), wants)


def test_scaled_stays_on_patch_gemm():
    """A SCALED call (z = relu(x * asc + ash) on load) at a shape the
    streaming kernel would take: with asc = 1, ash = 0 it is the conv of
    relu(x), exactly."""
    N, H, W, CI, KO = SHAPES["three_tiles"]
    x = _ints((N, H, W, CI), seed=11)
    w, taps = _onehot_fwd(KO, CI, 3)
    got = _run_ops({"s": ("scaled", "bf16", x, w, torch.ones(CI),
                          torch.zeros(CI))})["s"]
    _same(got, _expect_fwd(x.clamp_min(0), taps, KO, 3, 1, 1))
