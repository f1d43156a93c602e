// Cross-entropy: one fused fwd kernel (row max + logsumexp +
// NLL, one wave per row, shuffle reduction — guide Appendix B 'Reduction'),
// one bwd kernel (softmax - onehot, scaled). The soft-target pair next to
// them adds label smoothing and a two-label mix (CutMix/Mixup targets).
#include "common.h"

#include <climits>
#include <cstdint>

namespace {

template <typename T16>
__global__ void ce_fwd_kernel(const T16* __restrict__ logits,
                              const long* __restrict__ target,
                              float* __restrict__ loss,
                              float* __restrict__ lse, int B, int C) {
  const int b = blockIdx.x;  // one wave per row
  if (b >= B) return;
  const int lane = threadIdx.x;
  const T16* row = logits + (long)b * C;
  float mx = -3.4e38f;
  for (int c = lane; c < C; c += kWave) mx = fmaxf(mx, F16<T16>::to_f32(row[c]));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    mx = fmaxf(mx, __shfl_down(mx, off, kWave));
  mx = __shfl(mx, 0, kWave);
  float s = 0.f;
  for (int c = lane; c < C; c += kWave) s += __expf(F16<T16>::to_f32(row[c]) - mx);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, kWave);
  if (lane == 0) {
    const float l = mx + __logf(s);
    lse[b] = l;
    const long t = target[b];
    // out-of-range target: poison the loss (NaN) instead of faulting
    loss[b] = (t >= 0 && t < C) ? l - F16<T16>::to_f32(row[t])
                                : __builtin_nanf("");
  }
}

template <typename T16>
__global__ void ce_bwd_kernel(const T16* __restrict__ logits,
                              const long* __restrict__ target,
                              const float* __restrict__ lse,
                              const float* __restrict__ dloss,  // 0-dim, device
                              T16* __restrict__ dlogits, int B, int C,
                              float inv_b) {
  const float scale = (dloss ? *dloss : 1.f) * inv_b;
  const long total = (long)B * C;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (long)gridDim.x * blockDim.x) {
    const int c = (int)(t % C);
    const int b = (int)(t / C);
    float p = __expf(F16<T16>::to_f32(logits[t]) - lse[b]);
    if (c == (int)target[b]) p -= 1.f;
    dlogits[t] = F16<T16>::from_f32(p * scale);
  }
}

// Soft-target pair: label smoothing eps and a two-label mix per row,
//   loss_b = lam*nll(y_a) + (1-lam)*nll(y_b),
//   nll(t) = (1-eps)*(lse - z_t) + eps*(lse - mean_c z_c).
// y_b == nullptr stands for y_a and lam == nullptr for 1 (a plain target
// with smoothing). Targets and lam are read here, on the device, so a
// captured step follows new batches.
template <typename T16>
__global__ void ce_soft_fwd_kernel(const T16* __restrict__ logits,
                                   const long* __restrict__ ya,
                                   const long* __restrict__ yb,
                                   const float* __restrict__ lam,
                                   double* __restrict__ loss,
                                   float* __restrict__ lse, int B, int C,
                                   float eps) {
  const int b = blockIdx.x;  // one wave per row
  if (b >= B) return;
  const int lane = threadIdx.x;
  const T16* row = logits + (long)b * C;
  // pass 1: row max and the logit sum (for the smoothing term) together
  float mx = -3.4e38f, zs = 0.f;
  for (int c = lane; c < C; c += kWave) {
    const float z = F16<T16>::to_f32(row[c]);
    mx = fmaxf(mx, z);
    zs += z;
  }
  // the lanes' partial logit sums meet in double: 16-bit values summed in
  // fp32 per lane lose little, the cross-lane tree would lose more
  double zsd = (double)zs;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    mx = fmaxf(mx, __shfl_down(mx, off, kWave));
    zsd += __shfl_down(zsd, off, kWave);
  }
  mx = __shfl(mx, 0, kWave);
  float s = 0.f;
  for (int c = lane; c < C; c += kWave) s += __expf(F16<T16>::to_f32(row[c]) - mx);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, kWave);
  if (lane == 0) {
    // Once per row, so in double and with the precise log: the row's loss
    // is built from six products, and in fp32 each would round (the
    // hard-label kernel has one subtraction there). The rows stay double
    // for the mean, which then rounds to fp32 once. The hot pass above
    // keeps the fast __expf.
    const double l = (double)mx + log((double)s);
    lse[b] = (float)l;
    const long ta = ya[b];
    const long tb = yb ? yb[b] : ta;
    const double w = lam ? (double)lam[b] : 1.0;
    const double e = (double)eps;
    // out-of-range target in either slot: poison the loss (NaN), never
    // use it as an address
    if (ta >= 0 && ta < C && tb >= 0 && tb < C) {
      const double smooth = e * (l - zsd / (double)C);
      const double na =
          (1.0 - e) * (l - (double)F16<T16>::to_f32(row[ta])) + smooth;
      const double nb =
          (1.0 - e) * (l - (double)F16<T16>::to_f32(row[tb])) + smooth;
      loss[b] = w * na + (1.0 - w) * nb;
    } else {
      loss[b] = __builtin_nan("");
    }
  }
}

// what a row of the soft backward needs: lse, the two targets and the
// weights (1-eps)*lam, (1-eps)*(1-lam) of their one-hots
struct SoftRow {
  float lse, wa, wb;
  long ta, tb;
};

DEV_INLINE SoftRow soft_row(int b, const long* ya, const long* yb,
                            const float* lam, const float* lse, float eps) {
  SoftRow r;
  r.lse = lse[b];
  r.ta = ya[b];
  r.tb = yb ? yb[b] : r.ta;
  const float w = lam ? lam[b] : 1.f;
  r.wa = (1.f - eps) * w;
  r.wb = (1.f - eps) * (1.f - w);
  return r;
}

// dlogits = (softmax - q) * dloss / B,
//   q_c = eps/C + (1-eps)*(lam*[c==y_a] + (1-lam)*[c==y_b]).
// 8 elements per lane, 16 B loads and stores when `vec` (both buffers 16 B
// aligned); a lane's 8 elements may cross rows, the row state follows by
// carry. A target outside [0,C) matches no column.
template <typename T16>
__global__ void ce_soft_bwd_kernel(const T16* __restrict__ logits,
                                   const long* __restrict__ ya,
                                   const long* __restrict__ yb,
                                   const float* __restrict__ lam,
                                   const float* __restrict__ lse,
                                   const float* __restrict__ dloss,  // 0-dim
                                   T16* __restrict__ dlogits, int B, int C,
                                   float inv_b, float eps, float eps_c,
                                   bool vec) {
  const float scale = (dloss ? *dloss : 1.f) * inv_b;
  const long total = (long)B * C;
  const long nthr = (long)gridDim.x * blockDim.x;
  for (long e0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 8; e0 < total;
       e0 += nthr * 8) {
    int b = (int)(e0 / C);
    int c = (int)(e0 - (long)b * C);
    const int cnt = (int)(total - e0 < 8 ? total - e0 : 8);
    const bool full = vec && cnt == 8;
    short8 in;
    if (full) {
      in = *reinterpret_cast<const short8*>(logits + e0);
    } else {
      const short* ls = reinterpret_cast<const short*>(logits + e0);
#pragma unroll
      for (int u = 0; u < 8; ++u) in[u] = u < cnt ? ls[u] : (short)0;
    }
    SoftRow r = soft_row(b, ya, yb, lam, lse, eps);
    short8 o;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const float p = __expf(s16_to_f32<T16>(in[u]) - r.lse);
      const float q = eps_c + ((long)c == r.ta ? r.wa : 0.f) +
                      ((long)c == r.tb ? r.wb : 0.f);
      o[u] = f32_to_s16<T16>((p - q) * scale);
      if (++c == C) {
        c = 0;
        // past the end the walk stays on the last row; not stored
        b = min(b + 1, B - 1);
        r = soft_row(b, ya, yb, lam, lse, eps);
      }
    }
    if (full) {
      *reinterpret_cast<short8*>(dlogits + e0) = o;
    } else {
      short* ds = reinterpret_cast<short*>(dlogits + e0);
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (u < cnt) ds[u] = o[u];
    }
  }
}

void check_soft_args(const at::Tensor& logits, const at::Tensor& y_a,
                     const c10::optional<at::Tensor>& y_b,
                     const c10::optional<at::Tensor>& lam, double eps) {
  CHECK_GPU(logits);
  CHECK_CONTIG(logits);
  CHECK_16BIT(logits);
  TORCH_CHECK(logits.dim() == 2 && logits.size(0) >= 1 && logits.size(1) >= 1 &&
                  logits.size(0) <= INT_MAX && logits.size(1) <= INT_MAX,
              "logits must be (B,C) with B, C >= 1");
  TORCH_CHECK(eps >= 0.0 && eps <= 1.0, "label_smoothing must be in [0, 1], got ",
              eps);
  const long B = logits.size(0);
  auto check_target = [&](const at::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.device() == logits.device() &&
                    t.is_contiguous() && t.scalar_type() == at::kLong &&
                    t.dim() == 1 && t.size(0) == B,
                name, " must be a contiguous (B,) int64 tensor on the logits' "
                      "device");
  };
  check_target(y_a, "y_a");
  if (y_b) check_target(*y_b, "y_b");
  if (lam)
    TORCH_CHECK(lam->is_cuda() && lam->device() == logits.device() &&
                    lam->is_contiguous() && lam->scalar_type() == at::kFloat &&
                    lam->dim() == 1 && lam->size(0) == B,
                "lam must be a contiguous (B,) float32 tensor on the logits' "
                "device");
}

}  // namespace

std::vector<at::Tensor> cross_entropy_soft_fwd(
    at::Tensor logits, at::Tensor y_a, c10::optional<at::Tensor> y_b,
    c10::optional<at::Tensor> lam, double eps) {
  check_soft_args(logits, y_a, y_b, lam, eps);
  const int B = logits.size(0), C = logits.size(1);
  auto loss = at::empty({B}, logits.options().dtype(at::kDouble));
  auto lse = at::empty({B}, logits.options().dtype(at::kFloat));
  DISPATCH_16(logits, T16, {
    hipLaunchKernelGGL(ce_soft_fwd_kernel<T16>, dim3(B), dim3(kWave), 0,
                       cur_stream(), (const T16*)logits.data_ptr(),
                       y_a.data_ptr<long>(),
                       y_b ? y_b->data_ptr<long>() : nullptr,
                       lam ? lam->data_ptr<float>() : nullptr,
                       loss.data_ptr<double>(), lse.data_ptr<float>(), B, C,
                       (float)eps);
  });
  // the mean over rows in double, one rounding to the fp32 loss
  return {loss.mean().to(at::kFloat), lse};
}

// dloss as in cross_entropy_bwd: 0-dim fp32, read on the device; empty => 1.
at::Tensor cross_entropy_soft_bwd(at::Tensor logits, at::Tensor y_a,
                                  c10::optional<at::Tensor> y_b,
                                  c10::optional<at::Tensor> lam,
                                  at::Tensor lse, at::Tensor dloss,
                                  double eps) {
  check_soft_args(logits, y_a, y_b, lam, eps);
  const int B = logits.size(0), C = logits.size(1);
  TORCH_CHECK(lse.is_cuda() && lse.is_contiguous() &&
                  lse.scalar_type() == at::kFloat && lse.numel() == B,
              "lse must be (B,) float32 on GPU");
  TORCH_CHECK(dloss.numel() == 0 ||
                  (dloss.is_cuda() && dloss.scalar_type() == at::kFloat &&
                   dloss.numel() == 1),
              "dloss must be empty or one float32 element on GPU");
  auto dlogits = at::empty_like(logits);
  const long total = (long)B * C;
  const int grid =
      (int)std::max<long>(1, std::min<long>(cdiv_l(total, 256 * 8), 2048));
  const float* dl = dloss.numel() ? dloss.data_ptr<float>() : nullptr;
  const bool vec = ((uintptr_t)logits.data_ptr() % 16 == 0) &&
                   ((uintptr_t)dlogits.data_ptr() % 16 == 0);
  DISPATCH_16(logits, T16, {
    hipLaunchKernelGGL(ce_soft_bwd_kernel<T16>, dim3(grid), dim3(256), 0,
                       cur_stream(), (const T16*)logits.data_ptr(),
                       y_a.data_ptr<long>(),
                       y_b ? y_b->data_ptr<long>() : nullptr,
                       lam ? lam->data_ptr<float>() : nullptr,
                       lse.data_ptr<float>(), dl, (T16*)dlogits.data_ptr(), B,
                       C, 1.f / B, (float)eps, (float)eps / C, vec);
  });
  return dlogits;
}

std::vector<at::Tensor> cross_entropy_fwd(at::Tensor logits,
                                          at::Tensor target) {
  CHECK_GPU(logits);
  CHECK_CONTIG(logits);
  CHECK_16BIT(logits);
  const int B = logits.size(0), C = logits.size(1);
  auto loss = at::empty({B}, logits.options().dtype(at::kFloat));
  auto lse = at::empty({B}, logits.options().dtype(at::kFloat));
  DISPATCH_16(logits, T16, {
    hipLaunchKernelGGL(ce_fwd_kernel<T16>, dim3(B), dim3(kWave), 0,
                       cur_stream(), (const T16*)logits.data_ptr(),
                       target.data_ptr<long>(), loss.data_ptr<float>(),
                       lse.data_ptr<float>(), B, C);
  });
  return {loss.mean(), lse};
}

// dloss: 0-dim fp32 CUDA tensor (the upstream grad) read ON DEVICE so the
// backward is hipGraph-capturable (no host .item() sync); empty => 1.0.
at::Tensor cross_entropy_bwd(at::Tensor logits, at::Tensor target,
                             at::Tensor lse, at::Tensor dloss) {
  CHECK_GPU(logits);
  const int B = logits.size(0), C = logits.size(1);
  auto dlogits = at::empty_like(logits);
  const long total = (long)B * C;
  const int grid = (int)std::min<long>(cdiv_l(total, 256), 2048);
  const float* dl = dloss.numel() ? dloss.data_ptr<float>() : nullptr;
  DISPATCH_16(logits, T16, {
    hipLaunchKernelGGL(ce_bwd_kernel<T16>, dim3(grid), dim3(256), 0,
                       cur_stream(), (const T16*)logits.data_ptr(),
                       target.data_ptr<long>(), lse.data_ptr<float>(), dl,
                       (T16*)dlogits.data_ptr(), B, C, 1.f / B);
  });
  return dlogits;
}
