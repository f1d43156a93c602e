"""The nine-tap wgrad at 4x4 (conv_wgrad_mfma_t9<4>: an m-step is four
whole images) through conv2d_wgrad: exact impulse responses at every image,
step and chunk edge, random inputs against the fp32 CPU reference,
bit-identity with the s3 kernel, and bit-repeatability."""

import os
import subprocess
import sys

import pytest
import torch

from tests.test_gpu_wgrad_rows import _case, _ref, _wgrad

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. impulse: one 1.0 in x, so every dw entry is one dy value or 0 ----

IMP = (320, 4, 4, 64, 64)  # N, H, W, C, K: M = 5120 -> two chunks of 2560,
#                            the boundary between images 159 and 160
IMPULSES = {
    # images 4k..4k+3 share an m-step; image 6 is in the middle of one
    "corner_top_left": (6, 0, 0),
    "corner_top_right": (6, 0, 3),
    "corner_bottom_left": (6, 3, 0),
    "corner_bottom_right": (6, 3, 3),
    "interior": (6, 2, 1),
    # image boundary inside a step: without the zero rows between images,
    # dy of the neighbouring image lands in entries that must be 0
    "image_last_row": (1, 3, 2),
    "image_first_row": (2, 0, 2),
    "step_last_row": (3, 3, 1),
    "step_first_row": (4, 0, 1),
    "chunk_last_row": (159, 3, 0),
    "chunk_first_row": (160, 0, 3),
    "first_pixel": (0, 0, 0),
    "last_pixel": (319, 3, 3),
}


@pytest.fixture(scope="module")
def impulse_dy():
    N, H, W, _, K = IMP
    g = torch.Generator().manual_seed(5)
    return torch.randn(N, H, W, K, generator=g).to(torch.bfloat16)


@pytest.mark.parametrize("name", list(IMPULSES))
def test_impulse_exact(name, impulse_dy):
    N, H, W, C, K = IMP
    n, p, q = IMPULSES[name]
    c0 = (7 * list(IMPULSES).index(name) + 3) % C
    x = torch.zeros(N, H, W, C, dtype=torch.bfloat16)
    x[n, p, q, c0] = 1.0
    dw = _wgrad(x.cuda(), impulse_dy.cuda()).cpu()
    assert dw.shape == (K, C, 3, 3) and dw.dtype == torch.float32
    want = torch.zeros(K, C, 3, 3)
    for r in range(3):
        for s in range(3):
            pp, qq = p - r + 1, q - s + 1
            if 0 <= pp < H and 0 <= qq < W:
                want[:, c0, r, s] = impulse_dy[n, pp, qq].float()
    bad = (dw != want).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} wrong entries, first {bad[0]}"


# ---- 2. random inputs against the fp32 CPU reference -------------------

# max |dw - ref| allowed: twice what the s3 kernel (MI355X_WGRAD_T9=0)
# measured against the same reference at the same inputs. Measured (the
# nine-tap kernel gave the same figures, and the same bits; they are 1 to
# 6 ulp of the largest entries, which are about 4):
#   one_step 4.7684e-07, two_chunks 2.3842e-06, two_chunks_fp16 2.8610e-06,
#   two_c_tiles 7.1526e-07, two_k_tiles 7.1526e-07, bench_channels
#   1.1921e-06, six_images_s3 7.1526e-07
IMG4_CASES = {
    # name: (N, H, W, C, K, dtype, bound)
    "one_step": (4, 4, 4, 64, 64, torch.bfloat16, 9.5368e-07),
    "two_chunks": (320, 4, 4, 64, 64, torch.bfloat16, 4.7684e-06),
    "two_chunks_fp16": (320, 4, 4, 64, 64, torch.float16, 5.7220e-06),
    "two_c_tiles": (8, 4, 4, 128, 64, torch.bfloat16, 1.4305e-06),
    "two_k_tiles": (8, 4, 4, 64, 128, torch.bfloat16, 1.4305e-06),
    "bench_channels": (8, 4, 4, 512, 512, torch.bfloat16, 2.3842e-06),
    # N % 4 != 0: not eligible, stays on the s3 kernel
    "six_images_s3": (6, 4, 4, 64, 64, torch.bfloat16, 1.4305e-06),
}


@pytest.mark.parametrize("name", list(IMG4_CASES))
def test_random_vs_cpu(name):
    N, H, W, C, K, dtype, bound = IMG4_CASES[name]
    x, dy = _case(N, H, W, C, K, dtype)
    dw = _wgrad(x.cuda(), dy.cuda()).cpu()
    err = (dw - _ref(x.float(), dy.float())).abs().max().item()
    print(f"{name}: max abs err {err:.4e} (bound {bound})")
    assert err <= bound


# ---- 3. same bits as the s3 kernel, and from call to call ---------------

@pytest.fixture(scope="module")
def two_chunks():
    x, dy = _case(*IMG4_CASES["two_chunks"][:6])
    return x, dy, _wgrad(x.cuda(), dy.cuda())


S3_CHILD = """
import sys, torch
import mi355x.ops as ops
x, dy = torch.load(sys.argv[1])
dw = ops.ext().conv2d_wgrad(x.cuda(), dy.cuda(), 3, 3, 1, 1)
torch.save(dw.cpu(), sys.argv[2])
"""


def test_bit_identical_to_s3(two_chunks, tmp_path):
    """Same chunks, same natural position order inside a step: every dw
    element is the same sequence of MFMAs and slab adds as in the s3
    kernel, which a fresh process with the knob off runs."""
    x, dy, dw = two_chunks
    inp, out = str(tmp_path / "in.pt"), str(tmp_path / "dw_s3.pt")
    torch.save((x, dy), inp)
    r = subprocess.run([sys.executable, "-c", S3_CHILD, inp, out], cwd=REPO,
                       env=dict(os.environ, MI355X_WGRAD_T9="0"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + "\n" + r.stderr[-2500:]
    assert torch.equal(torch.load(out), dw.cpu())


def test_bit_repeatable(two_chunks):
    x, dy, dw = two_chunks
    assert torch.equal(_wgrad(x.cuda(), dy.cuda()), dw)
