"""The ring kernel of the 64-channel 3x3/s1 layer (conv_patch_ring: a block
keeps its weights in registers and walks whole images through a ring of
input rows) through conv2d_fwd, conv2d_fwd_stats and conv2d_dgrad: exact
placement with one-hot weights and with impulses at every step, image and
pad-column edge, exact BN statistics, the same bits as conv_patch_gemm,
random inputs against the fp32 CPU reference, and the routing predicate.

Knobs are read once per process, so the runs that need one (the old kernel,
MI355X_PATCH_RING=0; several images per block, MI355X_PATCH_RING_BLOCKS=2)
happen in two child processes, one per knob, shared by the tests."""

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

# name: (N, H, W, CI, KO). CI = 64 is the channel count of the tensor the
# kernel reads (x in fwd, dy in dgrad), KO that of the one it writes.
SHAPES = {
    "one_step": (1, 4, 32, 64, 64),     # one tile, both halo rows outside
    "two_steps": (3, 8, 32, 64, 64),    # rows handed from step to step
    "full_image": (2, 32, 32, 64, 64),  # 8 steps: the ring wraps twice
    "two_k_tiles": (2, 8, 32, 64, 128),
    "uneven_runs": (5, 8, 32, 64, 64),  # 2 blocks: 3 and 2 images
}
# the routing predicate: these stay on conv_patch_gemm
NOT_ELIGIBLE = {
    "h_not_4n": (2, 6, 32, 64, 64),
    "w16": (2, 16, 16, 64, 64),
    "ci128": (2, 8, 32, 128, 64),
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
        else:
            H, W = t[0].shape[1:3]
            out[key] = _dgrad(t[0], t[1], dtype, 1, 1, H, W,
                              t[2] if len(t) > 2 else None)
    return out


CHILD = """
import sys, torch
from tests.test_gpu_conv_ring import _run_ops
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


IMP_SHAPE = SHAPES["two_steps"]
# name: [(n, p, q), ...] of the 1.0s; with two blocks, block 0 runs image 0
# and then image 2
IMPULSES = {
    "step_first_pixel": [(1, 4, 0)],
    "step_last_pixel": [(1, 3, 31)],
    "image_first_row": [(1, 0, 5)],
    "image_last_row": [(1, 7, 20)],
    "pad_column_left": [(0, 2, 0)],
    "pad_column_right": [(0, 5, 31)],
    "image_change": [(0, 7, 9), (1, 0, 9), (2, 0, 9)],
}


def _impulse_case(name):
    """Impulse input, dense small-integer weights: every product and sum is
    a small integer, so F.conv2d in fp32 on the CPU is the exact answer."""
    N, H, W, CI, KO = IMP_SHAPE
    i = list(IMPULSES).index(name)
    a = torch.zeros(N, H, W, CI)
    for j, (n, p, q) in enumerate(IMPULSES[name]):
        a[n, p, q, (7 * i + 3 + 11 * j) % CI] = 1.0
    w = _ints((KO, CI, 3, 3), seed=40 + i, lo=-3, hi=3)
    addin = _ints((N, H, W, KO), seed=60 + i)
    an = a.permute(0, 3, 1, 2)
    y = F.conv2d(an, w, padding=1).permute(0, 2, 3, 1).contiguous()
    wt = w.permute(1, 0, 2, 3).contiguous()  # as dgrad weight: [K=CI, C=KO]
    dx = F.conv_transpose2d(an, wt, padding=1).permute(0, 2, 3, 1).contiguous()
    jobs = {f"imp-{name}-fwd": ("fwd", "bf16", a, w),
            f"imp-{name}-dgrad": ("dgrad", "bf16", a, wt),
            f"imp-{name}-addin": ("dgrad", "bf16", a, wt, addin)}
    wants = {f"imp-{name}-fwd": y, f"imp-{name}-dgrad": dx,
             f"imp-{name}-addin": dx + addin}
    return jobs, wants


def _once_case(dt):
    """ADDIN is added in fp32 and the sum rounded once (the check of
    test_gpu_conv_epilogue.test_addin_rounded_once, at 64 dy channels):
    acc = 1 + ulp/4 is exact in fp32; adding ulp/2 gives 1 + 0.75 ulp ->
    1 + ulp. Rounding acc first gives 1.0, then 1 + ulp/2 ties to 1.0."""
    ulp = 2.0 ** -7 if dt == "bf16" else 2.0 ** -10
    N, H, W, CI, KO = SHAPES["two_steps"]
    dy = torch.empty(N, H, W, CI)
    dy[..., :32] = 1.0
    dy[..., 32:] = ulp / 4
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


RAND = ["full_image", "two_k_tiles", "uneven_runs"]


def _rand_case(name, dt):
    """Random inputs, rounded to the dtype; fp32 CPU references."""
    N, H, W, CI, KO = SHAPES[name]
    g = torch.Generator().manual_seed(len(name) + len(dt) * 100 + KO)
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
    return _merge(_rand_case(n, dt) for n in RAND for dt in DT)


@pytest.fixture(scope="module")
def old_kernel(rand_cases, tmp_path_factory):
    """conv_patch_gemm on the random cases."""
    return _run_child(rand_cases[0], tmp_path_factory.mktemp("ring_off"),
                      MI355X_PATCH_RING="0")


@pytest.fixture(scope="module")
def two_blocks(rand_cases, tmp_path_factory):
    """Everything with two blocks per k-tile, so that a block runs several
    images and fetches the next image's rows during the last step of the
    current one: (jobs' results, wants of the exact cases)."""
    jobs, wants = _merge(
        [_place_case(f"{n}-{dt}", s, dt) for n, s in SHAPES.items()
         for dt in DT] + [_impulse_case(n) for n in IMPULSES] +
        [_once_case(dt) for dt in DT])
    jobs.update(rand_cases[0])
    got = _run_child(jobs, tmp_path_factory.mktemp("ring_2blocks"),
                     MI355X_PATCH_RING_BLOCKS="2")
    return got, wants


@pytest.fixture(scope="module")
def ring_rand(rand_cases):
    """The ring kernel on the random cases, a block per image."""
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

@pytest.mark.parametrize("name", ["two_steps", "full_image"])
def test_stats_exact(name):
    """Integers of |y| <= 8 over at most 2048 rows: every partial sum is an
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

def _ring_result(key, ring_rand, two_blocks):
    return two_blocks[0][key] if "uneven_runs" in key else ring_rand[key]


def _equal(a, b):
    if isinstance(a, tuple):
        return all(torch.equal(x, y) for x, y in zip(a, b))
    return torch.equal(a, b)


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("name", RAND)
def test_bit_identical_to_patch_gemm(name, dt, old_kernel, ring_rand,
                                     two_blocks):
    """Every output element is the same sequence of MFMAs (tap 0..8, kk
    0..3) and every stats row the same fold as in conv_patch_gemm, which a
    fresh process with MI355X_PATCH_RING=0 runs."""
    for op in ("fwd", "stats", "dgrad", "addin"):
        key = f"rand-{name}-{dt}-{op}"
        assert _equal(_ring_result(key, ring_rand, two_blocks),
                      old_kernel[key]), key
        if name != "uneven_runs":  # also a block per image == two blocks
            assert _equal(ring_rand[key], two_blocks[0][key]), key


def test_bit_repeatable(rand_cases, ring_rand):
    again = _run_ops(rand_cases[0])
    for key, got in ring_rand.items():
        assert _equal(again[key], got), key


# ---- 4. random inputs against the fp32 CPU reference ----------------------

# max |out - ref| allowed for (fwd, dgrad, dgrad + ADDIN): twice what
# conv_patch_gemm (MI355X_PATCH_RING=0) measured against the same reference
# at the same inputs. The ring kernel gave the same figures (and the same
# bits, test 3); they are half an ulp of the largest outputs, which are
# between 8 and 16 (ulp 2^-4 in bf16, 2^-7 in fp16). Measured:
MEASURED = {
    ("full_image", "bf16"): (3.1221e-02, 3.0998e-02, 3.1108e-02),
    ("full_image", "fp16"): (3.8710e-03, 3.7823e-03, 3.9062e-03),
    ("two_k_tiles", "bf16"): (3.0097e-02, 3.0861e-02, 3.1225e-02),
    ("two_k_tiles", "fp16"): (3.8624e-03, 3.8738e-03, 3.8443e-03),
    ("uneven_runs", "bf16"): (2.9881e-02, 3.0967e-02, 3.0878e-02),
    ("uneven_runs", "fp16"): (3.8052e-03, 3.3913e-03, 3.8214e-03),
}


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("name", RAND)
def test_random_vs_cpu(name, dt, rand_cases, old_kernel, ring_rand,
                       two_blocks):
    refs = rand_cases[1]
    for op, measured in zip(("fwd", "dgrad", "addin"), MEASURED[name, dt]):
        key = f"rand-{name}-{dt}-{op}"
        err = lambda t: (t - refs[key]).abs().max().item()
        e_new = err(_ring_result(key, ring_rand, two_blocks))
        print(f"{key}: max abs err {e_new:.4e}, conv_patch_gemm "
              f"{err(old_kernel[key]):.4e}, bound 2 x {measured}")
        assert e_new <= 2 * measured


# ---- 5. not eligible: stays on conv_patch_gemm ----------------------------

@pytest.mark.parametrize("name", list(NOT_ELIGIBLE))
def test_not_eligible_placement(name):
    jobs, wants = _place_case(name, NOT_ELIGIBLE[name], "bf16")
    _check(_run_ops(jobs), wants)
