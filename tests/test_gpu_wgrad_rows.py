"""The nine-tap row-stage wgrad (conv_wgrad_mfma_t9) through conv2d_wgrad:
exact impulse responses at every row/column/chunk edge, random inputs
against the fp32 CPU reference, bit-repeatability, and the shapes that
must keep taking the older kernels."""

import math

import pytest
import torch

import mi355x.ops as ops

pytestmark = pytest.mark.gpu


def _wgrad(x, dy):
    return ops.ext().conv2d_wgrad(x, dy, 3, 3, 1, 1)


# ---- 1. impulse: one 1.0 in x, so every dw entry is one dy value or 0 ----

IMP = (5, 32, 32, 64, 64)  # N, H, W, C, K: M = 5120 -> two chunks of 2560,
#                            the boundary between rows 15 and 16 of image 2
IMPULSES = {
    "corner_top_left": (3, 0, 0),
    "corner_top_right": (3, 0, 31),
    "corner_bottom_left": (3, 31, 0),
    "corner_bottom_right": (3, 31, 31),
    "mid_row_q0": (1, 13, 0),
    "mid_row_q31": (1, 13, 31),
    "step_last_row": (1, 5, 7),    # an m-step is two rows: (4,5) | (6,7)
    "step_first_row": (1, 6, 7),
    "chunk_last_row": (2, 15, 9),
    "chunk_first_row": (2, 16, 9),
    "last_row_last_image": (4, 31, 17),
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

def _ref(xc, dyc):
    """fp32 CPU wgrad of NHWC x / dy, as [K, C, 3, 3]."""
    w = torch.zeros(dyc.shape[3], xc.shape[3], 3, 3, requires_grad=True)
    y = torch.nn.functional.conv2d(xc.permute(0, 3, 1, 2), w, padding=1)
    y.backward(dyc.permute(0, 3, 1, 2))
    return w.grad


def _case(N, H, W, C, K, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H, W, C, generator=g).to(dtype)
    # 1/sqrt(M): dw entries are O(1), so one dropped row of W products
    # (about sqrt(W/M) of an entry) stands far above the rounding error
    dy = (torch.randn(N, H, W, K, generator=g) / math.sqrt(N * H * W)).to(
        dtype)
    return x, dy


def _max_err(x, dy):
    dw = _wgrad(x.cuda(), dy.cuda()).cpu()
    return (dw - _ref(x.float(), dy.float())).abs().max().item()


# max |dw - ref| allowed: twice what the s3 kernel (MI355X_WGRAD_T9=0)
# measured against the same reference at the same inputs. Measured (the
# nine-tap kernel gave the same five figures; they are 1 to 8 ulp of the
# largest entries, which are about 4):
#   img_per_step 4.7684e-07, four_rows_odd_n 2.1458e-06, two_c_tiles
#   1.9073e-06, two_chunks 3.8147e-06, two_chunks_fp16 3.9339e-06
ROW_CASES = {
    # name: (N, H, W, C, K, dtype, bound)
    "img_per_step": (2, 8, 8, 64, 64, torch.bfloat16, 9.5368e-07),
    "four_rows_odd_n": (3, 16, 16, 64, 128, torch.bfloat16, 4.2916e-06),
    "two_c_tiles": (1, 32, 32, 128, 64, torch.bfloat16, 3.8146e-06),
    "two_chunks": (5, 32, 32, 64, 64, torch.bfloat16, 7.6294e-06),
    "two_chunks_fp16": (5, 32, 32, 64, 64, torch.float16, 7.8678e-06),
}


@pytest.mark.parametrize("name", list(ROW_CASES))
def test_random_vs_cpu(name):
    N, H, W, C, K, dtype, bound = ROW_CASES[name]
    err = _max_err(*_case(N, H, W, C, K, dtype))
    print(f"{name}: max abs err {err:.3e} (bound {bound})")
    assert err <= bound


# ---- 3. repeatability ---------------------------------------------------

def test_bit_repeatable():
    x, dy = _case(5, 32, 32, 64, 64, torch.bfloat16, seed=3)
    x, dy = x.cuda(), dy.cuda()
    assert torch.equal(_wgrad(x, dy), _wgrad(x, dy))


# ---- 4. shapes that keep the older kernels ------------------------------

@pytest.mark.parametrize("hw", [4, 12])
def test_fallback_shapes(hw):
    x, dy = _case(2, hw, hw, 64, 64, torch.bfloat16, seed=hw)
    err = _max_err(x, dy)
    print(f"{hw}x{hw}: max abs err {err:.3e}")
    # The products are exact in fp32; what differs is the order of M <= 288
    # fp32 additions, here and in the reference: each sum carries a
    # rounding error of about sqrt(M) * 2^-24 * |entry| ~ 1e-6 for entries
    # of up to 4, so the largest of 36864 differences stays under 1e-5
    # (measured 4.8e-07 at 4x4 and 9.5e-07 at 12x12 before this kernel)
    assert err <= 1e-5
