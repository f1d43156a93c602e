"""Functional op layer: HIP/CDNA4 kernels on GPU, plain-torch fp32 on CPU.

Activation layout on GPU is NHWC end to end (coalesced channel-minor access
for CDNA4 implicit-GEMM conv; see mi355x/csrc/). Parameters are stored in
the PyTorch-conventional shapes/dtypes ([K,C,R,S] fp32 conv weight, etc.) so
state_dicts interchange with the reference scripts
(/root/reference/cifar_example.py:92-93 checkpoint format); 16-bit KRSC
copies for the kernels are cached per parameter version.

CPU tensors run a plain differentiable fp32 torch path — this is both the
BASELINE config-1 (CPU) execution mode and the numerics reference that the
GPU kernels are unit-tested against. CUDA tensors REQUIRE the mi355x._C
extension (no silent PyTorch fallback on GPU).
"""

from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch
import torch.nn.functional as F

from ._ext import ext

BN_EPS = 1e-5

_ACT_NONE = 0
_ACT_RELU = 1


def compute_dtype() -> torch.dtype:
    """Current 16-bit compute dtype for GPU kernels (bf16 unless amp says fp16)."""
    from mi355x import amp

    return amp.get_compute_dtype()


# ---------------------------------------------------------------------------
# cached 16-bit weight copies
# ---------------------------------------------------------------------------

# Bumped by the optimizer after each step (flat-param in-place updates do not
# advance the per-parameter ._version, so the cache keys on both).
_cache_epoch = 0


def bump_cache_epoch() -> None:
    global _cache_epoch
    _cache_epoch += 1


def _w16_conv(weight: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """fp32 [K,C,R,S] parameter -> cached 16-bit [K,R,S,C] kernel copy."""
    key = (weight._version, _cache_epoch, dtype)
    cache = getattr(weight, "_mi355x_w16", None)
    if cache is not None and cache[0] == key:
        return cache[1]
    if weight.is_cuda:
        like = torch.empty(0, dtype=dtype, device=weight.device)
        K, C = weight.shape[0], weight.shape[1]
        if C % 64 != 0 and K % 64 == 0:
            # generic small-C MFMA path wants [KO, KGP] zero-padded
            w16 = ext().cast_permute_krsc_pad(weight.detach(), like)
        else:
            w16 = ext().cast_permute_krsc(weight.detach(), like)
    else:
        w16 = weight.detach().to(dtype).permute(0, 2, 3, 1).contiguous()
    weight._mi355x_w16 = (key, w16)
    return w16


def _w16_conv_flip(weight: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """fp32 [K,C,R,S] parameter -> cached 16-bit [R,S,C,K] transposed copy
    (wt[r,s,c,k] = w[k,c,r,s]) — the dgrad MFMA kernel's B-operand layout.
    No spatial flip: the kernel's transposed-window gather pairs source row
    (h+pad-r)/stride directly with weight tap r (conv_mfma.hip)."""
    key = (weight._version, _cache_epoch, dtype)
    cache = getattr(weight, "_mi355x_wflip", None)
    if cache is not None and cache[0] == key:
        return cache[1]
    if weight.is_cuda:
        wf = ext().cast_permute_rsck(
            weight.detach(), torch.empty(0, dtype=dtype, device=weight.device))
    else:
        wf = weight.detach().to(dtype).permute(2, 3, 1, 0).contiguous()
    weight._mi355x_wflip = (key, wf)
    return wf


def _w16_linear(weight: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """fp32 [N,K] parameter -> cached 16-bit [N,K] kernel copy."""
    key = (weight._version, _cache_epoch, dtype)
    cache = getattr(weight, "_mi355x_w16", None)
    if cache is not None and cache[0] == key:
        return cache[1]
    w16 = weight.detach().to(dtype).contiguous()
    weight._mi355x_w16 = (key, w16)
    return w16


def _w16_linear_t(weight: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """fp32 [N,K] parameter -> cached 16-bit [K,N] transpose (the MFMA
    dgrad's B operand: dx = dy @ w == gemm_nt(dy, wT))."""
    key = (weight._version, _cache_epoch, dtype)
    cache = getattr(weight, "_mi355x_wT", None)
    if cache is not None and cache[0] == key:
        return cache[1]
    wt = weight.detach().to(dtype).t().contiguous()
    weight._mi355x_wT = (key, wt)
    return wt


def _relu_mask_bwd(dy: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """dy masked by y>0, via the extension's elementwise kernel."""
    return ext().relu_bwd(dy.contiguous(), y)


# ---------------------------------------------------------------------------
# conv2d (NHWC implicit GEMM)
# ---------------------------------------------------------------------------


class _ConvFn(torch.autograd.Function):
    """want_stats: the conv epilogue additionally emits BN (sum,sumsq)
    per-channel statistics of its output (conv->BN fusion — skips the
    separate bn_stats pass). The stats output is marked non-differentiable:
    the BN backward formula already carries the full d(stats)/d(x) terms.
    """

    @staticmethod
    def forward(ctx, x, weight, bias, stride, padding, act, want_stats=False):
        dtype = x.dtype
        w16 = _w16_conv(weight, dtype)
        stats = None
        if want_stats:
            y, stats = ext().conv2d_fwd_stats(x, w16, stride, padding,
                                              weight.shape[2],
                                              weight.shape[3])
        else:
            b32 = bias.detach().float() if bias is not None else torch.empty(0, device=x.device)
            y = ext().conv2d_fwd(x, w16, b32, stride, padding, act,
                                 weight.shape[2], weight.shape[3])
        ctx.save_for_backward(x, w16, y)
        ctx.weight_ref = weight  # for the cached dgrad weight-flip
        ctx.conf = (stride, padding, act, bias is not None, weight.shape)
        if want_stats:
            if stats is None:
                stats = torch.empty(0, device=x.device, dtype=torch.float32)
            ctx.mark_non_differentiable(stats)
            return y, stats
        return y

    @staticmethod
    def backward(ctx, dy, *unused_stats_grad):
        x, w16, y = ctx.saved_tensors
        stride, padding, act, has_bias, wshape = ctx.conf
        dy = dy.contiguous()
        if act == _ACT_RELU:
            dy = _relu_mask_bwd(dy, y)
        dx = None
        if ctx.needs_input_grad[0]:
            wflip = _w16_conv_flip(ctx.weight_ref, dy.dtype)
            dx = ext().conv2d_dgrad(dy, wflip, stride, padding,
                                    x.shape[1], x.shape[2],
                                    torch.empty(0, device=x.device,
                                                dtype=x.dtype))
        dw = None
        if ctx.needs_input_grad[1]:
            # wgrad kernels emit fp32 [K,C,R,S] directly (parameter layout)
            dw = ext().conv2d_wgrad(x, dy, wshape[2], wshape[3], stride,
                                    padding)
        db = None
        if has_bias and ctx.needs_input_grad[2]:
            db = dy.float().sum(dim=(0, 1, 2))
        return dx, dw, db, None, None, None, None


class _ConvTapFn(torch.autograd.Function):
    """conv2d with a residual TAP: forward returns (y, tap) where tap
    aliases the input. A ResNet block feeds `tap` (not x) to its shortcut
    path, so the junction gradient arrives HERE as d_tap in the same
    backward call as dy and is fused into the dgrad epilogue
    (dx = dgrad(dy) + d_tap) — autograd's separate full-tensor add at the
    junction disappears (r50-224 profile: 19 adds/step, 4.7% of step).
    The addin kernel variant is a separate compile-time instantiation, so
    non-tap convs run the exact same code as before."""

    @staticmethod
    def forward(ctx, x, weight, stride, padding):
        w16 = _w16_conv(weight, x.dtype)
        e = torch.empty(0, device=x.device)
        y = ext().conv2d_fwd(x, w16, e, stride, padding, _ACT_NONE,
                             weight.shape[2], weight.shape[3])
        ctx.save_for_backward(x, w16)
        ctx.weight_ref = weight
        ctx.conf = (stride, padding, weight.shape)
        return y, x.view_as(x)

    @staticmethod
    def backward(ctx, dy, dtap):
        x, w16 = ctx.saved_tensors
        stride, padding, wshape = ctx.conf
        dy = dy.contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            wflip = _w16_conv_flip(ctx.weight_ref, dy.dtype)
            add = (dtap.contiguous() if dtap is not None
                   else torch.empty(0, device=x.device, dtype=x.dtype))
            dx = ext().conv2d_dgrad(dy, wflip, stride, padding,
                                    x.shape[1], x.shape[2], add)
        elif dtap is not None:
            dx = dtap
        dw = None
        if ctx.needs_input_grad[1]:
            dw = ext().conv2d_wgrad(x, dy, wshape[2], wshape[3], stride,
                                    padding)
        return dx, dw, None, None


def conv2d_tap(x, weight, stride=1, padding=0):
    """conv2d returning (y, tap): route the block's shortcut through `tap`
    so its gradient fuses into this conv's dgrad epilogue (GPU training,
    MFMA shapes only; CPU keeps the plain double-use add semantics)."""
    if (x.is_cuda and x.requires_grad and weight.shape[1] % 64 == 0
            and weight.shape[0] % 64 == 0):
        return _ConvTapFn.apply(x, weight, stride, padding)
    return conv2d(x, weight, None, stride, padding, None), x


class _ConvTapStatsFn(torch.autograd.Function):
    """_ConvTapFn + epilogue BN stats: (y, tap, stats[2,K]) — the lazy-BN
    block entry (conv1 with junction-grad tap and stats for bn1)."""

    @staticmethod
    def forward(ctx, x, weight, stride, padding):
        w16 = _w16_conv(weight, x.dtype)
        y, stats = ext().conv2d_fwd_stats(x, w16, stride, padding,
                                          weight.shape[2], weight.shape[3])
        if stats is None:
            stats = torch.empty(0, device=x.device, dtype=torch.float32)
        ctx.save_for_backward(x, w16)
        ctx.weight_ref = weight
        ctx.conf = (stride, padding, weight.shape)
        ctx.mark_non_differentiable(stats)
        return y, x.view_as(x), stats

    @staticmethod
    def backward(ctx, dy, dtap, _unused):
        x, w16 = ctx.saved_tensors
        stride, padding, wshape = ctx.conf
        dy = dy.contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            wflip = _w16_conv_flip(ctx.weight_ref, dy.dtype)
            add = (dtap.contiguous() if dtap is not None
                   else torch.empty(0, device=x.device, dtype=x.dtype))
            dx = ext().conv2d_dgrad(dy, wflip, stride, padding,
                                    x.shape[1], x.shape[2], add)
        elif dtap is not None:
            dx = dtap
        dw = None
        if ctx.needs_input_grad[1]:
            dw = ext().conv2d_wgrad(x, dy, wshape[2], wshape[3], stride,
                                    padding)
        return dx, dw, None, None


def conv2d_tap_stats(x, weight, stride=1, padding=0):
    """(y, tap, stats_or_None) — see _ConvTapStatsFn."""
    y, tap, stats = _ConvTapStatsFn.apply(x, weight, stride, padding)
    return y, tap, (stats if stats.numel() else None)


class _BNConvFn(torch.autograd.Function):
    """Lazy BN: the BatchNorm apply (normalize + affine + ReLU) is fused
    into the CONSUMING conv's A-side load — the normalized activation z
    is never materialized (saves one full read + write of the tensor per
    internal BN; the bn_apply pass was 6-10% of the r18/r50 step).

    forward(x=conv1 output, bn params, conv2 weight) -> conv2(relu(bn(x)))
    [+ epilogue stats for the NEXT BN]. backward recomputes the ReLU mask
    from x (z > 0  <=>  x*asc+ash > 0), runs conv2's dgrad/wgrad (wgrad
    re-applies the transform on its x loads) and the standard fused BN
    backward."""

    @staticmethod
    def forward(ctx, x, gamma, beta, conv_weight, running_mean, running_var,
                momentum, stats, process_group, stride, padding, want_stats):
        N, H, W, C = x.shape
        m_local = N * H * W
        s = stats if stats is not None else ext().bn_stats(x)
        m_total = m_local
        if process_group is not None:
            import torch.distributed as dist

            dist.all_reduce(s, group=process_group)
            m_total = m_local * dist.get_world_size(process_group)
        empty = torch.empty(0, device=x.device)
        mi = ext().bn_finalize(
            s, running_mean if running_mean is not None else empty,
            running_var if running_var is not None else empty,
            float(m_total), momentum, BN_EPS)
        mean, invstd = mi[0], mi[1]
        g32 = gamma.detach().float()
        asc = g32 * invstd
        ash = beta.detach().float() - mean * asc
        w16 = _w16_conv(conv_weight, x.dtype)
        y, stats2 = ext().conv2d_fwd_scaled(x, w16, asc, ash, stride,
                                            padding, want_stats)
        ctx.save_for_backward(x, w16, mean, invstd, gamma, asc, ash)
        ctx.weight_ref = conv_weight
        ctx.conf = (stride, padding, conv_weight.shape, m_total,
                    process_group)
        if want_stats:
            ctx.mark_non_differentiable(stats2)
            return y, stats2
        return y

    @staticmethod
    def backward(ctx, dy2, *unused_stats_grad):
        x, w16, mean, invstd, gamma, asc, ash = ctx.saved_tensors
        stride, padding, wshape, m_total, pg = ctx.conf
        dy2 = dy2.contiguous()
        efx = torch.empty(0, device=x.device, dtype=x.dtype)
        # conv2 backward w.r.t. the virtual z
        dw = None
        if ctx.needs_input_grad[3]:
            dw = ext().conv2d_wgrad_scaled(x, asc, ash, dy2, wshape[2],
                                           wshape[3], stride, padding)
        wflip = _w16_conv_flip(ctx.weight_ref, dy2.dtype)
        dz = ext().conv2d_dgrad(dy2, wflip, stride, padding, x.shape[1],
                                x.shape[2], efx)
        # fused BN backward with the ReLU mask recomputed from x
        emask = torch.empty(0, device=x.device, dtype=torch.uint8)
        r = ext().bn_bwd_reduce(x, dz, efx, mean, invstd, emask, asc, ash)
        if pg is not None:
            import torch.distributed as dist

            dist.all_reduce(r, group=pg)
        dgamma, dbeta = r[0], r[1]
        dx, _ = ext().bn_bwd_dx(x, dz, efx, mean, invstd,
                                gamma.detach().float(), dgamma, dbeta,
                                float(m_total), False, emask, asc, ash)
        return (dx, dgamma, dbeta, dw, None, None, None, None, None, None,
                None, None)


def bn_conv(x, gamma, beta, conv_weight, running_mean, running_var,
            momentum=0.1, stats=None, process_group=None, stride=1,
            padding=0, want_stats=False):
    """Fused BN(relu) -> conv2d (lazy-BN consumer fusion). Returns y, or
    (y, stats2) when want_stats. GPU/MFMA shapes only; callers gate."""
    return _BNConvFn.apply(x, gamma, beta, conv_weight, running_mean,
                           running_var, momentum, stats, process_group,
                           stride, padding, want_stats)


def conv2d_with_stats(x, weight, stride=1, padding=0):
    """GPU conv returning (y, bn_stats[2,C] or None) — the fused
    conv->BN entry used by the ResNet blocks. stats is None when the
    shape has no stats-emitting kernel path (caller falls back to
    bn_stats)."""
    return _ConvFn.apply(x, weight, None, stride, padding, _ACT_NONE, True)


def _check_depthwise(x, weight, stride, padding, groups):
    """The depthwise domain: every value outside it is named in a
    ValueError."""
    C = x.shape[-1]
    if groups != C:
        raise ValueError(
            f"conv2d: groups={groups} is not supported: only groups=1 and "
            f"groups == channels ({C}), the depthwise case")
    if weight.shape[0] != groups or weight.shape[1] != 1:
        raise ValueError(
            f"conv2d: a depthwise weight must be [{groups}, 1, R, R] "
            f"(channel multiplier 1), got {tuple(weight.shape)}")
    R, S = weight.shape[2], weight.shape[3]
    if R != S or R not in (3, 5):
        raise ValueError(
            f"conv2d: depthwise kernels are 3x3 or 5x5, got {R}x{S}")
    if stride not in (1, 2):
        raise ValueError(
            f"conv2d: depthwise stride must be 1 or 2, got {stride!r}")
    if not isinstance(padding, int) or not 0 <= padding <= R - 1:
        raise ValueError(
            f"conv2d: depthwise padding must be in [0, {R - 1}] for a "
            f"{R}x{R} kernel, got {padding!r}")


def conv2d(x, weight, bias=None, stride=1, padding=0, act=None, groups=1):
    """2-D convolution. x: NHWC; weight: fp32 [K,C/groups,R,S] (torch
    layout).

    act: None | 'relu' fused into the epilogue (and into the kernel backward
    mask). Reference call sites: /root/reference/cifar_example.py:20-29.

    groups: 1 (dense), or the channel count of x (depthwise: weight
    [C,1,R,R] with R in {3,5}, stride 1 or 2, padding <= R-1). Anything
    else raises ValueError. The depthwise case runs on the CPU path only:
    the kernel library has no depthwise kernel, so on the GPU it raises
    NotImplementedError (never an eager-torch fallback). A depthwise weight
    never reaches _w16_conv.
    """
    a = _ACT_RELU if act == "relu" else _ACT_NONE
    if groups != 1:
        _check_depthwise(x, weight, stride, padding, groups)
        if x.is_cuda:
            raise NotImplementedError(
                "conv2d: depthwise convolution (groups == channels) has no "
                "GPU kernel in this library yet; it runs on the CPU path "
                "only")
        y = F.conv2d(x.permute(0, 3, 1, 2), weight, bias, stride, padding,
                     groups=groups)
        y = y.permute(0, 2, 3, 1)
        return F.relu(y) if a == _ACT_RELU else y
    if x.is_cuda:
        return _ConvFn.apply(x, weight, bias, stride, padding, a)
    y = F.conv2d(x.permute(0, 3, 1, 2), weight, bias, stride, padding)
    y = y.permute(0, 2, 3, 1)
    if a == _ACT_RELU:
        y = F.relu(y)
    return y


# ---------------------------------------------------------------------------
# linear (MFMA GEMM)
# ---------------------------------------------------------------------------


class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, act):
        w16 = _w16_linear(weight, x.dtype)
        b32 = bias.detach().float() if bias is not None else torch.empty(0, device=x.device)
        y = ext().linear_fwd(x, w16, b32, act)
        ctx.save_for_backward(x, w16, y)
        ctx.weight_ref = weight  # for the cached dgrad transpose
        ctx.conf = (act, bias is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w16, y = ctx.saved_tensors
        act, has_bias = ctx.conf
        dy = dy.contiguous()
        if act == _ACT_RELU:
            dy = _relu_mask_bwd(dy, y)
        dx = None
        if ctx.needs_input_grad[0]:
            wt = _w16_linear_t(ctx.weight_ref, dy.dtype)
            dx = ext().linear_dgrad(dy, w16, wt)
        dw = ext().linear_wgrad(x, dy) if ctx.needs_input_grad[1] else None
        db = dy.float().sum(dim=0) if (has_bias and ctx.needs_input_grad[2]) else None
        return dx, dw, db, None


def linear(x, weight, bias=None, act=None):
    """y = x @ W^T + b. x: [M,K]; weight: fp32 [N,K]."""
    a = _ACT_RELU if act == "relu" else _ACT_NONE
    if x.is_cuda:
        return _LinearFn.apply(x, weight, bias, a)
    y = F.linear(x, weight, bias)
    if a == _ACT_RELU:
        y = F.relu(y)
    return y


# ---------------------------------------------------------------------------
# batch norm (+ residual add + relu, fused)
# ---------------------------------------------------------------------------


class _BNFn(torch.autograd.Function):
    """Training-mode batch norm over NHWC with optional fused residual add
    and ReLU. Stats in fp32. Optionally SyncBN: partial (sum,sumsq) and the
    backward (sum_dy, sum_dy_xhat) reductions are all-reduced over the
    process group (BASELINE config 5)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, residual, running_mean, running_var,
                momentum, act, process_group, stats=None):
        N, H, W, C = x.shape
        m_local = N * H * W
        # stats precomputed by the producing conv's epilogue when fused
        s = stats if stats is not None else ext().bn_stats(x)
        m_total = m_local
        if process_group is not None:
            import torch.distributed as dist

            dist.all_reduce(s, group=process_group)
            m_total = m_local * dist.get_world_size(process_group)
        empty = torch.empty(0, device=x.device)
        mi = ext().bn_finalize(
            s, running_mean if running_mean is not None else empty,
            running_var if running_var is not None else empty,
            float(m_total), momentum, BN_EPS)  # [2,C]: mean, invstd
        mean, invstd = mi[0], mi[1]
        res = residual if residual is not None else torch.empty(0, device=x.device, dtype=x.dtype)
        y, mask = ext().bn_apply(x, mean, invstd, gamma.detach().float(),
                                 beta.detach().float(), res, act, True)
        # mask: 1-bit-per-element "y > 0" (fast path + relu) — backward
        # reads it instead of re-reading y (1/16 the bytes)
        if mask is None:
            mask = torch.empty(0, device=x.device, dtype=torch.uint8)
        ctx.save_for_backward(x, y, mean, invstd, gamma, mask)
        ctx.conf = (act, residual is not None, m_total, process_group)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, mean, invstd, gamma, mask = ctx.saved_tensors
        act, has_res, m_total, pg = ctx.conf
        dy = dy.contiguous()
        # ReLU mask fused into both backward kernels (no standalone pass)
        y_arg = y if act == _ACT_RELU else torch.empty(0, device=x.device,
                                                       dtype=x.dtype)
        ef = torch.empty(0, device=x.device)
        r = ext().bn_bwd_reduce(x, dy, y_arg, mean, invstd, mask, ef, ef)
        if pg is not None:
            import torch.distributed as dist

            dist.all_reduce(r, group=pg)
        dgamma, dbeta = r[0], r[1]
        want_dres = has_res and act == _ACT_RELU
        dx, dres = ext().bn_bwd_dx(x, dy, y_arg, mean, invstd,
                                   gamma.detach().float(), dgamma, dbeta,
                                   float(m_total), want_dres, mask, ef, ef)
        if has_res and not want_dres:
            dres = dy  # no activation: residual grad is dy itself
        elif not has_res:
            dres = None
        return dx, dgamma, dbeta, dres, None, None, None, None, None, None


def batch_norm(x, gamma, beta, running_mean, running_var, training,
               momentum=0.1, residual=None, act=None, process_group=None,
               stats=None):
    """BatchNorm over NHWC with optional fused residual-add + ReLU.

    Matches torch BN semantics (momentum convention, unbiased running var).
    process_group != None => SyncBatchNorm (stats all-reduced over ranks).
    stats: precomputed (sum,sumsq) from the producing conv's epilogue.
    """
    a = _ACT_RELU if act == "relu" else _ACT_NONE
    if x.is_cuda:
        if training:
            return _BNFn.apply(x, gamma, beta, residual, running_mean,
                               running_var, momentum, a, process_group,
                               stats)
        mean = running_mean.float()
        invstd = torch.rsqrt(running_var.float() + BN_EPS)
        res = residual if residual is not None else torch.empty(0, device=x.device, dtype=x.dtype)
        # eval: no backward, skip the relu-mask allocation + stores
        return ext().bn_apply(x.contiguous(), mean, invstd,
                              gamma.detach().float(), beta.detach().float(),
                              res, a, False)[0]
    xc = x.permute(0, 3, 1, 2)
    y = F.batch_norm(xc, running_mean, running_var, gamma, beta, training,
                     momentum, BN_EPS).permute(0, 2, 3, 1)
    if residual is not None:
        y = y + residual
    if a == _ACT_RELU:
        y = F.relu(y)
    return y


# ---------------------------------------------------------------------------
# pooling
# ---------------------------------------------------------------------------


class _MaxPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kernel, stride, padding):
        y, idx = ext().maxpool_fwd(x, kernel, stride, padding)
        ctx.save_for_backward(idx)
        ctx.conf = (x.shape, kernel, stride, padding)
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        xshape, kernel, stride, padding = ctx.conf
        dx = ext().maxpool_bwd(dy.contiguous(), idx, xshape[1], xshape[2],
                               kernel, stride, padding)
        return dx, None, None, None


def max_pool2d(x, kernel, stride=None, padding=0):
    """Max pooling over NHWC. Reference: /root/reference/cifar_example.py:21."""
    stride = stride or kernel
    if x.is_cuda:
        return _MaxPoolFn.apply(x, kernel, stride, padding)
    y = F.max_pool2d(x.permute(0, 3, 1, 2), kernel, stride, padding)
    return y.permute(0, 2, 3, 1)


class _GAPFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.conf = x.shape
        return ext().global_avg_pool(x)

    @staticmethod
    def backward(ctx, dy):
        N, H, W, C = ctx.conf
        dx = (dy / (H * W)).reshape(N, 1, 1, C).expand(N, H, W, C).contiguous()
        return dx


def global_avg_pool(x):
    """NHWC [N,H,W,C] -> [N,C] mean over H,W."""
    if x.is_cuda:
        return _GAPFn.apply(x)
    return x.mean(dim=(1, 2))


# ---------------------------------------------------------------------------
# loss
# ---------------------------------------------------------------------------


class _CEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        loss, lse = ext().cross_entropy_fwd(logits, target)
        ctx.save_for_backward(logits, target, lse)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        logits, target, lse = ctx.saved_tensors
        # dloss read on-device (hipGraph-capturable: no host sync)
        if not (torch.is_tensor(dloss) and dloss.is_cuda):
            dloss = torch.as_tensor(dloss, dtype=torch.float32,
                                    device=logits.device)
        dlogits = ext().cross_entropy_bwd(logits, target, lse,
                                          dloss.float().reshape(()))
        return dlogits, None


class MixTarget(NamedTuple):
    """Two labels per row and the weight of the first: what CutMix and
    Mixup train against. ``y_a``, ``y_b`` int64 (B,), ``lam`` float32 (B,),
    all on the logits' device. DeviceLoader yields one per batch when its
    Augment mixes; cross_entropy takes it in place of a label tensor."""

    y_a: torch.Tensor
    y_b: torch.Tensor
    lam: torch.Tensor

    def to(self, *args, **kwargs):
        return MixTarget(*(t.to(*args, **kwargs) for t in self))


class _SoftCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, y_a, y_b, lam, eps):
        loss, lse = ext().cross_entropy_soft_fwd(logits, y_a, y_b, lam, eps)
        ctx.save_for_backward(logits, y_a, lse)
        # y_b and lam may be None (a plain target): kept beside the saved
        # tensors, they need no grad and are never written in place by us
        ctx.rest = (y_b, lam, eps)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        logits, y_a, lse = ctx.saved_tensors
        y_b, lam, eps = ctx.rest
        # dloss read on-device (hipGraph-capturable: no host sync)
        if not (torch.is_tensor(dloss) and dloss.is_cuda):
            dloss = torch.as_tensor(dloss, dtype=torch.float32,
                                    device=logits.device)
        dlogits = ext().cross_entropy_soft_bwd(
            logits, y_a, y_b, lam, lse, dloss.float().reshape(()), eps)
        return dlogits, None, None, None, None


def cross_entropy(logits, target, label_smoothing=0.0):
    """Mean cross-entropy. logits [B,C] (16-bit on GPU), target int64 [B]
    or a MixTarget. Reference call site:
    /root/reference/cifar_example.py:63,78.

    With ``eps = label_smoothing`` the loss of a row is

        lam*nll(y_a) + (1-lam)*nll(y_b),
        nll(t) = (1-eps)*(lse - z_t) + eps*(lse - mean_c z_c)

    (a plain target is y_a = y_b, lam = 1): F.cross_entropy(...,
    label_smoothing=eps, reduction='none') mixed per row. GPU: one forward
    and one backward kernel; both targets, lam and the upstream gradient
    are read on the device, so a captured step follows new batches. A
    target outside [0,C) in either slot makes the loss NaN. With
    label_smoothing == 0 and a plain target this is the hard-label kernel
    pair, unchanged."""
    eps = float(label_smoothing)
    if not 0.0 <= eps <= 1.0:
        raise ValueError(f"label_smoothing must be in [0, 1], got {eps}")
    mixed = isinstance(target, MixTarget)
    if logits.is_cuda:
        if not mixed and eps == 0.0:
            return _CEFn.apply(logits, target)
        if mixed:
            return _SoftCEFn.apply(logits, target.y_a, target.y_b,
                                   target.lam, eps)
        return _SoftCEFn.apply(logits, target, None, None, eps)
    if not mixed and eps == 0.0:
        return F.cross_entropy(logits.float(), target)
    lp = F.log_softmax(logits.float(), dim=1)
    smooth = -lp.mean(dim=1)

    def nll(t):
        return (1.0 - eps) * -lp.gather(1, t[:, None])[:, 0] + eps * smooth

    if not mixed:
        return nll(target).mean()
    lam = target.lam.float()
    return (lam * nll(target.y_a) + (1.0 - lam) * nll(target.y_b)).mean()


# ---------------------------------------------------------------------------
# batch building from a device-resident uint8 dataset
# ---------------------------------------------------------------------------


def gather_augment(data_u8, targets, indices, scale, shift, *, pad=0,
                   flip=False, seed=0, epoch=0):
    """Build a batch from the uint8 NHWC dataset: gather ``indices``,
    zero-pad by ``pad`` and crop at a random offset, flip, then
    ``v*scale[c] + shift[c]`` (a padded pixel is raw 0, so it comes out as
    shift[c] — the torchvision crop -> flip -> normalize order). The draws
    are ``mi355x.data.augment_params(seed, epoch, indices, pad, flip)``.

    Returns (x NHWC, y int64). GPU: one kernel, x in the compute dtype,
    indices int32. CPU: fp32. pad=0, flip=False is the eval path (gather +
    normalize + layout only). No autograd.

    ``indices`` must lie in [0, N). The CPU path raises IndexError
    otherwise; the kernel cannot raise, so it reads nothing for such an
    index and returns an all-padding image with label -1 (which the
    cross-entropy kernel turns into a NaN loss). DeviceLoader checks the
    epoch's indices on the host before it launches anything.
    """
    if data_u8.is_cuda:
        like = torch.empty(0, dtype=compute_dtype(), device=data_u8.device)
        x, y = ext().gather_augment(data_u8, targets, indices, scale, shift,
                                    int(pad), bool(flip), int(seed),
                                    int(epoch), like)
        return x, y
    idx = indices.to(torch.int64)
    v = _gather_raw_cpu(data_u8, idx, pad, flip, seed, epoch,
                        "gather_augment")
    return v * scale + shift, targets[idx]


def _gather_raw_cpu(data_u8, idx, pad, flip, seed, epoch, who):
    """The CPU ops' gather + crop + flip, before normalization: float32
    (B,H,W,C) of raw byte values, a padded pixel 0."""
    from mi355x.data import augment_params

    N, H, W, _ = data_u8.shape
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= N):
        raise IndexError(f"{who}: index outside dataset of {N}")
    dy, dx, f = augment_params(seed, epoch, idx, pad, flip)
    sh = torch.arange(H)[None, :] + (dy[:, None] - pad)             # (B,H)
    ww = torch.arange(W)[None, :]
    sw = torch.where(f[:, None] != 0, W - 1 - ww, ww) + (dx[:, None] - pad)
    ok = ((sh >= 0) & (sh < H))[:, :, None] & ((sw >= 0) & (sw < W))[:, None, :]
    v = data_u8[idx[:, None, None], sh.clamp(0, H - 1)[:, :, None],
                sw.clamp(0, W - 1)[:, None, :]]                     # (B,H,W,C)
    return v.to(torch.float32) * ok[..., None]


def mix_thresholds(cutmix, mixup):
    """The 16-bit mode thresholds (Tc, Tm) = round(p*65536) of the cutmix
    and mixup probabilities; the kernel and the numpy twin both take them
    from here."""
    cutmix, mixup = float(cutmix), float(mixup)
    if not (0.0 <= cutmix <= 1.0 and 0.0 <= mixup <= 1.0
            and cutmix + mixup <= 1.0):
        raise ValueError("cutmix and mixup must be probabilities with "
                         f"cutmix + mixup <= 1, got {cutmix} and {mixup}")
    tc, tm = int(round(cutmix * 65536)), int(round(mixup * 65536))
    return tc, min(tm, 65536 - tc)


def gather_augment_mix(data_u8, targets, indices, scale, shift, *, pad=0,
                       flip=False, cutmix=0.0, mixup=0.0, seed=0, epoch=0):
    """gather_augment with CutMix / Mixup: returns (x NHWC, y_a, y_b, lam).

    Call A[b] what gather_augment builds for batch position b before it
    normalizes (own crop and flip, padding raw 0). Position b's partner is
    position B-1-b of the same call (the middle of an odd batch and B=1 pair
    with themselves). Each position draws, from the hash of its own dataset
    index (``mi355x.data.mix_params``), cutmix with probability ``cutmix``,
    mixup with probability ``mixup``, else nothing:

      none    x = A[b]                          lam = 1        y_b = y_a
      cutmix  x = A[B-1-b] inside a box,        lam = kept     y_b = the
              A[b] outside                      area / (H*W)   partner's
      mixup   x = lam*A[b] + (1-lam)*A[B-1-b]   lam = u/65536  label

    then ``v*scale[c] + shift[c]`` and one rounding, as gather_augment. lam
    is uniform on [0,1): Beta(1,1), the CIFAR setting of both papers; a
    general Beta(alpha) is not supported. The cutmix box has sides
    sqrt(1-lam0)*(H,W) around a uniform centre and is clipped to the image;
    lam is the area kept after the clip.

    GPU: one kernel (one byte gather per none/cutmix element, two per mixup
    element), x in the compute dtype, indices int32. CPU: fp32, bit-equal
    before the rounding to 16 bits. Out-of-range indices: as
    gather_augment (CPU raises IndexError; the kernel reads nothing for
    them and gives label -1 in the slot concerned). No autograd.
    """
    tc, tm = mix_thresholds(cutmix, mixup)
    N, H, W, _ = data_u8.shape
    inv_hw = float(np.float32(1.0 / (H * W)))
    if data_u8.is_cuda:
        like = torch.empty(0, dtype=compute_dtype(), device=data_u8.device)
        return tuple(ext().gather_augment_mix(
            data_u8, targets, indices, scale, shift, int(pad), bool(flip),
            tc, tm, inv_hw, int(seed), int(epoch), like))
    from mi355x.data import MIX_CUT, MIX_NONE, MIX_UP, mix_params

    idx = indices.to(torch.int64)
    a = _gather_raw_cpu(data_u8, idx, pad, flip, seed, epoch,
                        "gather_augment_mix")
    p = a.flip(0)                                  # A[B-1-b]
    mode, box, lam = mix_params(seed, epoch, idx, H, W, cutmix, mixup)
    hh = torch.arange(H)[None, :, None]
    ww = torch.arange(W)[None, None, :]
    inbox = ((mode == MIX_CUT)[:, None, None]
             & (hh >= box[:, 0, None, None]) & (hh < box[:, 1, None, None])
             & (ww >= box[:, 2, None, None]) & (ww < box[:, 3, None, None]))
    v = torch.where(inbox[..., None], p, a)
    w = lam[:, None, None, None]
    # fp32, and exact: see the kernel's comment
    v = torch.where((mode == MIX_UP)[:, None, None, None],
                    a * w + p * (1.0 - w), v)
    y_a = targets[idx]
    y_b = torch.where(mode == MIX_NONE, y_a, y_a.flip(0))
    return v * scale + shift, y_a, y_b, lam


# ---------------------------------------------------------------------------
# fused optimizer step
# ---------------------------------------------------------------------------


def sgd_step(flat_param, flat_grad, flat_momentum, lr, momentum,
             weight_decay=0.0, grad_scale=1.0):
    """v = mu*v + (g*gs + wd*p); p -= lr*v — one kernel over the flat fp32
    buffers (reference semantics: optim.SGD(lr,momentum),
    /root/reference/cifar_example.py:64)."""
    if flat_param.is_cuda:
        ext().sgd_step(flat_param, flat_grad, flat_momentum, lr, momentum,
                       weight_decay, grad_scale)
        return
    g = flat_grad.mul(grad_scale)
    if weight_decay != 0.0:
        g = g.add(flat_param, alpha=weight_decay)
    flat_momentum.mul_(momentum).add_(g)
    flat_param.add_(flat_momentum, alpha=-lr)


# ---------------------------------------------------------------------------
# guarded optimizer step: global-norm clipping + device-side loss scaling
# ---------------------------------------------------------------------------

# Guard state: one float32[8] tensor (layout: mi355x/csrc/gradstat.hip).
# The integer fields hold int32 bit patterns: read them through
# state.view(torch.int32).
GS_SCALE, GS_INV_SCALE, GS_TRACKER, GS_SKIPPED = 0, 1, 2, 3
GS_NONFINITE, GS_RAW_NORM, GS_LAST_NORM, GS_LAST_COEF = 4, 5, 6, 7
GS_LEN = 8
GRAD_STATS_SLAB = 2 * 2048  # floats: per-block sums of squares, then counts


def new_guard_state(device, scale=1.0):
    """A fresh guard state: the given loss scale, every counter zero."""
    st = torch.zeros(GS_LEN, dtype=torch.float32)
    st[GS_SCALE] = scale
    st[GS_INV_SCALE] = 1.0 / scale
    st[GS_LAST_COEF] = 1.0
    return st.to(device)


def grad_stats(flat_grad, slab=None, out=None):
    """L2 norm and inf/nan element count of the flat fp32 grad buffer, left
    on the device: returns (norm 0-d float32, count 0-d int32), views of
    ``out`` (float32[2]: count bits, norm; allocated if None).

    GPU: one pass of per-block partials into ``slab`` (float32
    [GRAD_STATS_SLAB], allocated if None), then a fixed-order one-block
    combine in double, so two calls on one buffer agree bit for bit. An
    element counts as non-finite by its own exponent bits (a finite value
    whose square overflows does not), like ``torch.isfinite``."""
    if out is None:
        out = torch.empty(2, dtype=torch.float32, device=flat_grad.device)
    if flat_grad.is_cuda:
        if slab is None:
            slab = torch.empty(GRAD_STATS_SLAB, dtype=torch.float32,
                               device=flat_grad.device)
        ext().grad_stats(flat_grad, slab, out)
    else:
        iout = out.view(torch.int32)
        iout[0] = (~torch.isfinite(flat_grad)).sum().clamp(max=2**31 - 1)
        out[1] = flat_grad.double().square().sum().sqrt()
    return out[1], out.view(torch.int32)[0]


def _guard_coef(state, grad_scale, max_norm):
    """(norm, coef, eff) as float32 0-d tensors — gradstat.hip's guard_coef."""
    k = state[GS_INV_SCALE] * torch.tensor(grad_scale, dtype=torch.float32,
                                           device=state.device)
    norm = state[GS_RAW_NORM] * k
    if max_norm == float("inf"):
        coef = torch.ones_like(norm)
    else:
        # fminf semantics: a nan quotient (skipped step anyway) gives 1
        q = torch.tensor(max_norm, dtype=torch.float32,
                         device=state.device) / (norm + 1e-6)
        coef = torch.where(q < 1.0, q, torch.ones_like(q))
    return norm, coef, k * coef


def _lr_tensor(lr, flat_param, who):
    """lr as the update kernels take it: None for a float, else the checked
    one-element float32 tensor on the buffers' device."""
    if not isinstance(lr, torch.Tensor):
        return None
    if (lr.numel() != 1 or lr.dtype != torch.float32
            or lr.device != flat_param.device):
        raise ValueError(f"{who}: a tensor lr must be one float32 element "
                         "on the buffers' device")
    return lr


def _check_ema(ema, clock, flat_param, who):
    if ema is None:
        return
    if clock is None:
        raise ValueError(f"{who}: an EMA update needs the step clock")
    if (ema.shape != flat_param.shape or ema.dtype != torch.float32
            or ema.device != flat_param.device):
        raise ValueError(f"{who}: ema must be float32 with the parameters' "
                         "shape and device")
    if (clock.numel() < CK_LEN or clock.dtype != torch.float32
            or clock.device != flat_param.device):
        raise ValueError(f"{who}: the clock must be float32[{CK_LEN}] on the "
                         "buffers' device")


def _ema_update_cpu(ema, flat_param, clock):
    """e += omd * (w - e): the CPU form of csrc/guard.h's ema_elem."""
    ema.add_(flat_param - ema, alpha=float(clock[CK_EMA_OMD]))


def sgd_step_guarded(flat_param, flat_grad, flat_momentum, state, lr,
                     momentum, weight_decay=0.0, grad_scale=1.0,
                     max_norm=float("inf"), ema=None, clock=None):
    """sgd_step with the gradient multiplier taken from the guard ``state``
    that grad_stats filled (state[4:6]):

        norm = raw_norm * grad_scale * inv_scale   (the true gradient's norm)
        coef = min(1, max_norm / (norm + 1e-6))    (1 if max_norm is inf)
        g_eff = g * (grad_scale * inv_scale * coef) + wd * p

    and nothing written at all if the gradient holds an inf/nan. No host
    sync on the GPU. With inv_scale == 1 and max_norm == inf this is
    sgd_step bit for bit.

    ``lr`` is a float or a 0-d float32 tensor on the buffers' device (the
    clock's CK_LR slot under a schedule), read when the kernel runs; the
    arithmetic is the same either way. With ``ema`` (float32, the
    parameters' layout) the same pass also does ``e += omd * (w_new - e)``,
    omd = ``clock[CK_EMA_OMD]``; a skipped step leaves ``ema`` alone too."""
    max_norm = float(max_norm)
    lr_t = _lr_tensor(lr, flat_param, "sgd_step_guarded")
    _check_ema(ema, clock, flat_param, "sgd_step_guarded")
    if flat_param.is_cuda:
        ext().sgd_step_guarded(flat_param, flat_grad, flat_momentum, state,
                               lr_t, 0.0 if lr_t is not None else lr,
                               momentum, weight_decay, grad_scale, max_norm,
                               ema, clock if ema is not None else None)
        return
    if int(state.view(torch.int32)[GS_NONFINITE]) != 0:
        return
    _, _, eff = _guard_coef(state, grad_scale, max_norm)
    g = flat_grad.mul(eff)
    if weight_decay != 0.0:
        g = g.add(flat_param, alpha=weight_decay)
    flat_momentum.mul_(momentum).add_(g)
    flat_param.add_(flat_momentum, alpha=-float(lr))
    if ema is not None:
        _ema_update_cpu(ema, flat_param, clock)


def scaler_update(state, grad_scale=1.0, max_norm=float("inf"),
                  growth_factor=2.0, backoff_factor=0.5, growth_interval=0):
    """After sgd_step_guarded: GradScaler.step_ok's rules applied to the
    guard state on the device. Overflow: scale *= backoff, tracker = 0,
    skipped += 1. Clean: tracker += 1, and at growth_interval scale *= growth,
    tracker = 0. growth_interval <= 0 keeps the scale (clip-only use). Also
    stores the step's norm and clip coefficient for logging."""
    max_norm = float(max_norm)
    if state.is_cuda:
        ext().scaler_update(state, grad_scale, max_norm, growth_factor,
                            backoff_factor, int(growth_interval))
        return
    norm, coef, _ = _guard_coef(state, grad_scale, max_norm)
    ist = state.view(torch.int32)
    if int(ist[GS_NONFINITE]) != 0:
        ist[GS_SKIPPED] += 1
        if growth_interval > 0:
            state[GS_SCALE] *= backoff_factor
            ist[GS_TRACKER] = 0
    elif growth_interval > 0:
        ist[GS_TRACKER] += 1
        if int(ist[GS_TRACKER]) >= growth_interval:
            state[GS_SCALE] *= growth_factor
            ist[GS_TRACKER] = 0
    state[GS_INV_SCALE] = 1.0 / state[GS_SCALE]
    state[GS_LAST_NORM] = norm
    state[GS_LAST_COEF] = coef


# ---------------------------------------------------------------------------
# step clock: learning-rate schedule and EMA weight, advanced on the device
# ---------------------------------------------------------------------------

# Step clock: one float32[4] tensor (layout: mi355x/csrc/gradstat.hip).
# CK_STEP holds an int32 bit pattern: read it through clock.view(torch.int32).
CK_STEP, CK_LR, CK_EMA_OMD = 0, 1, 2
CK_LEN = 4


def ema_one_minus_decay(step, ema_decay, ema_warmup):
    """1 - d_t for applied-step number ``step``: d_t = ema_decay, or
    min(ema_decay, (1 + t) / (10 + t)) with the warm-up. Computed in double
    (a Python float); storing it into the float32 clock rounds it once, as
    clock_advance_kernel does."""
    d = float(ema_decay)
    if ema_warmup:
        d = min(d, (1.0 + step) / (10.0 + step))
    return 1.0 - d


def clock_set(clock, step, table, ema_decay=0.0, ema_warmup=False):
    """Host write of the clock for ``step`` applied steps: what a new
    optimizer (step 0) and a checkpoint load do. In place."""
    step = int(step)
    if not 0 <= step < 2 ** 31:
        raise ValueError(f"clock_set: step {step} outside int32")
    host = torch.zeros(CK_LEN, dtype=torch.float32)
    host.view(torch.int32)[CK_STEP] = step
    host[CK_LR] = table[min(step, table.numel() - 1)]
    host[CK_EMA_OMD] = ema_one_minus_decay(step, ema_decay, ema_warmup)
    clock.copy_(host)
    return clock


def new_clock(device, table, ema_decay=0.0, ema_warmup=False):
    """A step clock at step 0 for the float32 schedule ``table``."""
    return clock_set(torch.empty(CK_LEN, dtype=torch.float32, device=device),
                     0, table, ema_decay, ema_warmup)


def clock_advance(clock, state, table, ema_decay=0.0, ema_warmup=False):
    """After scaler_update: count the step on the device and look up what
    the next one uses. If ``state`` (a guard state, or None) reports a
    non-finite gradient, nothing moves. Otherwise

        t = ++clock[CK_STEP]
        clock[CK_LR] = table[min(t, T-1)]
        clock[CK_EMA_OMD] = 1 - d_t          (ema_one_minus_decay)

    ``table`` is a float32 tensor of T >= 1 learning rates on the clock's
    device. GPU: one thread, no host sync."""
    if (table.dim() != 1 or table.numel() < 1 or table.dtype != torch.float32
            or table.device != clock.device):
        raise ValueError("clock_advance: the table must be a non-empty 1-D "
                         "float32 tensor on the clock's device")
    if clock.is_cuda:
        ext().clock_advance(clock, state, table, float(ema_decay),
                            bool(ema_warmup))
        return
    if (state is not None
            and int(state.view(torch.int32)[GS_NONFINITE]) != 0):
        return
    ick = clock.view(torch.int32)
    t = min(max(int(ick[CK_STEP]), -1) + 1, 2 ** 31 - 1)
    ick[CK_STEP] = t
    clock[CK_LR] = table[min(t, table.numel() - 1)]
    clock[CK_EMA_OMD] = ema_one_minus_decay(t, ema_decay, ema_warmup)


# ---------------------------------------------------------------------------
# LARS: per-tensor norms and trust ratios over the flat buffers
# ---------------------------------------------------------------------------

LARS_TILE = 4096  # elements; kTile in mi355x/csrc/lars.hip
LARS_MAX_TENSORS = 2048  # kMaxTensors there: the finalise block's LDS
LARS_WNORM, LARS_GNORM, LARS_TRUST = 0, 1, 2  # columns of plan.stats


class LarsPlan:
    """What the LARS kernels need to know about the flat layout (layout of
    the tables: mi355x/csrc/lars.hip). Built once by lars_plan.

      table  int32 [T, 4]   tiles: {start, length, tensor, 0}
      tens   int32 [S, 4]   tensors: {first tile, past last tile, excluded, 0}
      slab   float32 [3*T]  pass 1's per-tile partials (GPU only)
      stats  float32 [S, 3] per tensor: ||w_s||, raw ||g_s||, trust_s
    """

    def __init__(self, offsets, exclude, device):
        offsets = [int(o) for o in offsets]
        exclude = [bool(e) for e in exclude]
        if len(offsets) < 2 or offsets[0] != 0:
            raise ValueError("lars_plan: offsets must be S+1 ints from 0")
        if any(b < a for a, b in zip(offsets, offsets[1:])):
            raise ValueError("lars_plan: offsets must ascend")
        if len(exclude) != len(offsets) - 1:
            raise ValueError(f"lars_plan: {len(offsets) - 1} tensors but "
                             f"{len(exclude)} exclude flags")
        if len(exclude) > LARS_MAX_TENSORS:
            raise ValueError(f"lars_plan: {len(exclude)} tensors, at most "
                             f"{LARS_MAX_TENSORS} are supported")
        if offsets[-1] >= 2 ** 31 - 1:
            raise ValueError("lars_plan: 2^31 elements or more")
        self.offsets, self.exclude = offsets, exclude
        self.numel = offsets[-1]
        self.device = torch.device(device)
        tiles, tens = [], []
        for s, (a, b) in enumerate(zip(offsets, offsets[1:])):
            first = len(tiles)
            tiles.extend((t, min(LARS_TILE, b - t), s, 0)
                         for t in range(a, b, LARS_TILE))
            tens.append((first, len(tiles), int(exclude[s]), 0))
        S, T = len(tens), len(tiles)
        self.table = torch.tensor(tiles, dtype=torch.int32).reshape(T, 4).to(
            self.device)
        self.tens = torch.tensor(tens, dtype=torch.int32).to(self.device)
        self.slab = torch.empty(3 * T, dtype=torch.float32,
                                device=self.device)
        self.stats = torch.zeros(S, 3, dtype=torch.float32,
                                 device=self.device)
        self.stats[:, LARS_TRUST] = 1.0
        # CPU fallback: per-element expansion of per-tensor values
        self._sizes = torch.tensor([b - a for a, b in zip(offsets, offsets[1:])])
        self._excluded = torch.tensor(exclude)

    def check(self, *flats):
        for f in flats:
            if f.dim() != 1 or f.numel() != self.numel:
                raise ValueError(
                    f"LARS plan ends at element {self.numel} but the flat "
                    f"buffer has shape {tuple(f.shape)}")

    def per_element(self, per_tensor):
        return torch.repeat_interleave(per_tensor, self._sizes)


def lars_plan(offsets, exclude, device):
    """Plan for lars_stats/lars_step: ``offsets`` are the S+1 ascending
    element offsets of the S tensors in the flat buffers (0 first, numel
    last), ``exclude`` S bools (True: trust 1 and no weight decay). Tensors
    may start at any element and have any size; at most LARS_MAX_TENSORS
    (2048) tensors and fewer than 2^31 elements."""
    return LarsPlan(offsets, exclude, device)


def lars_stats(flat_param, flat_grad, plan, state, grad_scale=1.0,
               max_norm=float("inf"), weight_decay=0.0, eta=1e-3, eps=1e-8):
    """One pass over ``flat_param`` and ``flat_grad``: the global raw norm
    and inf/nan count of the gradient into ``state[4:6]`` (as grad_stats
    leaves them) and, per tensor of the plan, into ``plan.stats``:

        wn_s = ||w_s||,  raw ||g_s||,
        trust_s = eta*wn_s / (gn_s + wd*wn_s + eps),  gn_s = ||g_s|| * eff
                  (1 for an excluded tensor, or if wn_s or gn_s is 0)

    with eff the guarded step's multiplier grad_scale*inv_scale*clip_coef.
    GPU: per-tile partials, then one fixed-order combine in double: two
    calls on the same buffers agree bit for bit. Returns plan.stats."""
    max_norm = float(max_norm)
    plan.check(flat_param, flat_grad)
    if flat_param.is_cuda:
        ext().lars_stats(flat_param, flat_grad, plan.table, plan.tens,
                         plan.slab, state, plan.stats, grad_scale, max_norm,
                         weight_decay, eta, eps)
        return plan.stats
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    S = len(plan.exclude)
    sums = torch.zeros(S, 2, dtype=torch.float64)
    for s, (a, b) in enumerate(zip(plan.offsets, plan.offsets[1:])):
        sums[s, 0] = flat_param[a:b].double().square().sum()
        sums[s, 1] = flat_grad[a:b].double().square().sum()
    state.view(torch.int32)[GS_NONFINITE] = (
        ~torch.isfinite(flat_grad)).sum().clamp(max=2**31 - 1)
    state[GS_RAW_NORM] = sums[:, 1].sum().sqrt()
    _, _, eff = _guard_coef(state, grad_scale, max_norm)
    # float32, one rounding per op, in lars.hip's trust_ratio order
    wn = sums[:, 0].sqrt().float()
    gn_raw = sums[:, 1].sqrt().float()
    gn = gn_raw * eff
    den = (gn + f32(weight_decay) * wn) + f32(eps)
    trust = (f32(eta) * wn) / den
    keep = (wn > 0) & (gn > 0) & ~plan._excluded
    plan.stats[:, LARS_WNORM] = wn
    plan.stats[:, LARS_GNORM] = gn_raw
    plan.stats[:, LARS_TRUST] = torch.where(keep, trust, torch.ones_like(trust))
    return plan.stats


def lars_step(flat_param, flat_grad, flat_momentum, plan, state, lr,
              momentum, weight_decay=0.0, grad_scale=1.0,
              max_norm=float("inf"), ema=None, clock=None):
    """The LARS update with the trust ratios lars_stats left in the plan:

        gr = g * eff + wd_s * w        (wd_s = 0 for an excluded tensor)
        m  = mu * m + trust_s * gr
        w -= lr * m

    and nothing written at all if the gradient holds an inf/nan. ``lr`` is
    a float or a 0-d float32 tensor on the buffers' device, read when the
    kernel runs: a captured step then follows ``lr.fill_(v)`` or the step
    clock's schedule. With ``ema`` (float32, the parameters' layout) the
    same pass also does ``e += omd * (w_new - e)``, omd =
    ``clock[CK_EMA_OMD]``; a skipped step leaves ``ema`` alone too."""
    max_norm = float(max_norm)
    plan.check(flat_param, flat_grad, flat_momentum)
    lr_t = _lr_tensor(lr, flat_param, "lars_step")
    _check_ema(ema, clock, flat_param, "lars_step")
    if flat_param.is_cuda:
        ext().lars_step(flat_param, flat_grad, flat_momentum, plan.table,
                        plan.tens, state, plan.stats, lr_t,
                        0.0 if lr_t is not None else lr, momentum,
                        weight_decay, grad_scale, max_norm, ema,
                        clock if ema is not None else None)
        return
    if int(state.view(torch.int32)[GS_NONFINITE]) != 0:
        return
    _, _, eff = _guard_coef(state, grad_scale, max_norm)
    wd = torch.where(plan._excluded, 0.0, float(weight_decay)).float()
    gr = flat_grad.mul(eff).add_(plan.per_element(wd) * flat_param)
    gr.mul_(plan.per_element(plan.stats[:, LARS_TRUST]))
    flat_momentum.mul_(momentum).add_(gr)
    flat_param.sub_(flat_momentum * (lr_t.reshape(()) if lr_t is not None
                                     else lr))
    if ema is not None:
        _ema_update_cpu(ema, flat_param, clock)


# ---------------------------------------------------------------------------
# device-side meter: loss / top-k / confusion counts with no host read
# ---------------------------------------------------------------------------

# Meter state: one int64[8] tensor (layout: mi355x/csrc/meter.hip).
# MT_LOSS_SUM holds a float64 bit pattern: read it through
# state[MT_LOSS_SUM:MT_LOSS_SUM + 1].view(torch.float64).
MT_ROWS, MT_CORRECT1, MT_CORRECTK, MT_BAD, MT_LOSS_SUM, MT_UPDATES = range(6)
MT_LEN = 8
METER_MAX_BLOCKS = 2048            # kMaxBlocks in meter.hip
METER_SLAB = 4 * METER_MAX_BLOCKS  # int64: nll sums (float64 bits), 3 counts


def _meter_nll_sum(nll, C):
    """The sum of the rows' nll (float64 (B,), 0 for a bad row) in the order
    meter.hip adds it for C columns: per row group over the grid's passes,
    the block's groups in order, then meter_finalise_kernel's order."""
    B = nll.numel()
    rpb = 256 // (16 if C <= 16 else 64)          # rows per block pass
    grid = max(1, min(-(-B // rpb), METER_MAX_BLOCKS))
    per_pass = grid * rpb
    passes = -(-B // per_pass)
    x = F.pad(nll, (0, passes * per_pass - B)).reshape(passes, grid, rpb)
    acc = x[0]
    for p in range(1, passes):                     # a group's rows, in turn
        acc = acc + x[p]
    blk = acc[:, 0]
    for j in range(1, rpb):                        # the block's groups
        blk = blk + acc[:, j]
    y = F.pad(blk, (0, METER_MAX_BLOCKS - grid)).reshape(-1, 256)
    t = y[0]
    for j in range(1, y.shape[0]):                 # thread t: t, t+256, ...
        t = t + y[j]
    w = t.reshape(4, 64)
    lane = torch.arange(64, device=w.device)
    for off in (32, 16, 8, 4, 2, 1):               # the xor butterfly
        w = w + w[:, lane ^ off]
    return (w[0, 0] + w[1, 0]) + (w[2, 0] + w[3, 0])


def _meter_update_torch(state, logits, y_a, y_b, lam, k, loss, confusion):
    """meter.hip's decisions in plain torch, on the logits' device, with no
    host read."""
    B, C = logits.shape
    z = logits.detach().float()
    t = y_a if y_b is None else torch.where(lam >= 0.5, y_a, y_b)
    t_ok = (t >= 0) & (t < C)
    ts = torch.where(t_ok, t, torch.zeros_like(t))  # never index with a bad one
    zt = z.gather(1, ts[:, None])                   # (B,1)
    mx = z.max(dim=1, keepdim=True).values
    col = torch.arange(C, device=z.device)[None, :]
    pred = torch.where(z == mx, col, C).min(dim=1).values
    lse = (mx + (z - mx).exp().sum(dim=1, keepdim=True).log())[:, 0]
    good = t_ok & torch.isfinite(lse)
    rank = ((z > zt) | ((z == zt) & (col < ts[:, None]))).sum(dim=1)
    nll = torch.where(good, (lse - zt[:, 0]).double(),
                      torch.zeros((), dtype=torch.float64, device=z.device))
    if loss is not None:
        add = loss.detach().reshape(()).float().double() * float(B)
    else:
        add = _meter_nll_sum(nll, C)
    state[MT_ROWS] += B
    state[MT_CORRECT1] += (good & (rank == 0)).sum()
    state[MT_CORRECTK] += (good & (rank < k)).sum()
    state[MT_BAD] += (~good).sum()
    state[MT_LOSS_SUM:MT_LOSS_SUM + 1].view(torch.float64).add_(add)
    state[MT_UPDATES] += 1
    if confusion is not None:
        cell = torch.where(good, ts * C + pred.clamp(max=C - 1),
                           torch.zeros_like(ts))
        confusion.view(-1).index_add_(0, cell, good.to(torch.int64))


def meter_update(state, slab, logits, y_a, y_b=None, lam=None, *, k,
                 loss=None, confusion=None):
    """Add one batch to a meter ``state`` (int64[MT_LEN], layout in
    mi355x/csrc/meter.hip), on the logits' device and with no host read.

    logits (B,C); the row's label is ``y_a``, or with a mix target
    ``lam >= 0.5 ? y_a : y_b``. Per row: lse and nll = lse - z_t (fp32, the
    hard-label loss kernel's arithmetic), pred = the first index of the row
    maximum, rank = #{c : z_c > z_t} + #{c < t : z_c == z_t}. A row is bad
    if its label lies outside [0,C) or its lse is not finite; it counts in
    rows and bad and nowhere else. A good row is correct@1 if rank == 0,
    correct@k if rank < k, adds its nll to the loss sum and one to
    ``confusion[t, pred]`` (int64 (C,C), optional). With ``loss`` (0-d
    float32 on the device, the batch's mean loss as the training loop has
    it) the loss sum takes ``double(loss) * B`` instead of the rows' nll.

    16-bit logits on the GPU: two kernels, per-block partials in ``slab``
    (int64[METER_SLAB]) combined in one fixed order, so two runs agree bit
    for bit. CPU tensors, and GPU logits that are not 16-bit, run plain
    torch ops that make the same decisions: counts and matrix equal the
    kernel's, and so does the loss sum under ``loss=``."""
    k = int(k)
    if k < 1:
        raise ValueError(f"meter_update: k must be at least 1, got {k}")
    if logits.dim() != 2 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise ValueError("meter_update: logits must be (B,C) with B, C >= 1")
    if (y_b is None) != (lam is None):
        raise ValueError("meter_update: y_b and lam come together")
    if logits.is_cuda and logits.dtype in (torch.bfloat16, torch.float16):
        if loss is not None:
            loss = loss.detach().reshape(())
            if loss.dtype != torch.float32:
                loss = loss.float()
        ext().meter_update(state, slab, logits.detach(), y_a, y_b, lam, k,
                           loss, confusion, 0)
        return
    _meter_update_torch(state, logits, y_a, y_b, lam, k, loss, confusion)
