// Linear layer GEMMs. The classifier GEMMs in this
// workload are small ([B,512]x[512,10] for ResNet-18/CIFAR); these are
// simple coalesced direct kernels, kept as the fallback for shapes the
// MFMA tile path (gemm_mfma.hip) does not cover.
#include "common.h"

namespace {

// y[M,N] = x[M,K] @ w[N,K]^T + b
template <typename T16>
__global__ void linear_fwd_kernel(const T16* __restrict__ x,
                                  const T16* __restrict__ w,
                                  const float* __restrict__ bias,
                                  T16* __restrict__ y, int M, int N, int K,
                                  int act, int has_bias) {
  const long total = (long)M * N;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (long)gridDim.x * blockDim.x) {
    const int nn = (int)(t % N);
    const int m = (int)(t / N);
    const T16* xp = x + (long)m * K;
    const T16* wp = w + (long)nn * K;
    float acc = has_bias ? bias[nn] : 0.f;
    int k = 0;
    if (K % 8 == 0) {
      for (; k < K; k += 8) {
        short8 xv = *reinterpret_cast<const short8*>(xp + k);
        short8 wv = *reinterpret_cast<const short8*>(wp + k);
#pragma unroll
        for (int u = 0; u < 8; ++u)
          acc += s16_to_f32<T16>(xv[u]) * s16_to_f32<T16>(wv[u]);
      }
    } else {
      for (; k < K; ++k)
        acc += F16<T16>::to_f32(xp[k]) * F16<T16>::to_f32(wp[k]);
    }
    if (act == 1) acc = relu_f(acc);
    y[t] = F16<T16>::from_f32(acc);
  }
}

// dx[M,K] = dy[M,N] @ w[N,K]
template <typename T16>
__global__ void linear_dgrad_kernel(const T16* __restrict__ dy,
                                    const T16* __restrict__ w,
                                    T16* __restrict__ dx, int M, int N,
                                    int K) {
  const long total = (long)M * K;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (long)gridDim.x * blockDim.x) {
    const int k = (int)(t % K);
    const int m = (int)(t / K);
    float acc = 0.f;
    for (int nn = 0; nn < N; ++nn)
      acc += F16<T16>::to_f32(dy[(long)m * N + nn]) *
             F16<T16>::to_f32(w[(long)nn * K + k]);
    dx[t] = F16<T16>::from_f32(acc);
  }
}

// dw[N,K] (f32) = dy[M,N]^T @ x[M,K]; split-M over blockIdx.y, one
// partial [N,K] row per chunk folded in a fixed order by fold_rows
// (classifier dw is small, the M loop is the long axis)
template <typename T16>
__global__ void linear_wgrad_kernel(const T16* __restrict__ x,
                                    const T16* __restrict__ dy,
                                    float* __restrict__ dw, int M, int N,
                                    int K, int m_per_chunk) {
  const long total = (long)N * K;
  const int m0 = blockIdx.y * m_per_chunk;
  const int m1 = min(M, m0 + m_per_chunk);
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (long)gridDim.x * blockDim.x) {
    const int k = (int)(t % K);
    const int nn = (int)(t / K);
    float acc = 0.f;
    for (int m = m0; m < m1; ++m)
      acc += F16<T16>::to_f32(dy[(long)m * N + nn]) *
             F16<T16>::to_f32(x[(long)m * K + k]);
    dw[(long)blockIdx.y * total + t] = acc;
  }
}

inline int ggrid(long n) { return (int)std::min<long>(cdiv_l(n, 256), 4096); }

}  // namespace

at::Tensor gemm_nt_mfma(at::Tensor A, at::Tensor B, at::Tensor bias, long act,
                        bool out32);  // gemm_mfma.hip

at::Tensor linear_fwd(at::Tensor x, at::Tensor w, at::Tensor bias, long act) {
  CHECK_GPU(x);
  CHECK_CONTIG(x);
  CHECK_16BIT(x);
  const int M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(w.size(1) == K, "linear weight/input mismatch");
  // MFMA tile path once there is at least one K-slice and a few M-tiles;
  // direct kernel keeps the sub-MFMA shapes (K % 8 != 0 or tiny M)
  if (K % 8 == 0 && K >= 64 && M >= 128)
    return gemm_nt_mfma(x, w, bias, act, false);
  auto y = at::empty({M, N}, x.options());
  const int has_bias = bias.numel() > 0;
  DISPATCH_16(x, T16, {
    hipLaunchKernelGGL(linear_fwd_kernel<T16>, dim3(ggrid((long)M * N)),
                       dim3(256), 0, cur_stream(), (const T16*)x.data_ptr(),
                       (const T16*)w.data_ptr(),
                       has_bias ? bias.data_ptr<float>() : nullptr,
                       (T16*)y.data_ptr(), M, N, K, (int)act, has_bias);
  });
  return y;
}

// wt (optional, may be empty): cached [K,N] transpose of w — the MFMA
// dgrad runs dx = dy @ w as gemm_nt(dy, wT) when the N reduction is
// MFMA-sized.
at::Tensor linear_dgrad(at::Tensor dy, at::Tensor w, at::Tensor wt) {
  CHECK_GPU(dy);
  CHECK_CONTIG(dy);
  const int M = dy.size(0), N = dy.size(1), K = w.size(1);
  if (wt.numel() > 0 && N % 8 == 0 && N >= 64 && M >= 128) {
    auto none = at::empty({0}, dy.options().dtype(at::kFloat));
    return gemm_nt_mfma(dy, wt, none, 0, false);
  }
  auto dx = at::empty({M, K}, dy.options());
  DISPATCH_16(dy, T16, {
    hipLaunchKernelGGL(linear_dgrad_kernel<T16>, dim3(ggrid((long)M * K)),
                       dim3(256), 0, cur_stream(), (const T16*)dy.data_ptr(),
                       (const T16*)w.data_ptr(), (T16*)dx.data_ptr(), M, N,
                       K);
  });
  return dx;
}

at::Tensor linear_wgrad(at::Tensor x, at::Tensor dy) {
  CHECK_GPU(x);
  CHECK_CONTIG(x);
  const int M = x.size(0), K = x.size(1), N = dy.size(1);
  // dw = dy^T @ x as gemm_nt(dyT, xT) with the M reduction in the MFMA
  // K-slot; the two transposes are tiny next to the M-long reduction
  if (M % 8 == 0 && M >= 256 && N >= 32 && K >= 64) {
    auto dyT = dy.t().contiguous();
    auto xT = x.t().contiguous();
    auto none = at::empty({0}, x.options().dtype(at::kFloat));
    return gemm_nt_mfma(dyT, xT, none, 0, true);
  }
  const long total = (long)N * K;
  const long xy_blocks = cdiv_l(total, 256);
  int nchunks = (int)std::min<long>(std::max<long>(512 / xy_blocks, 1),
                                    cdiv_l(M, 64));
  const int m_per_chunk = (int)cdiv_l(M, nchunks);
  nchunks = (int)cdiv_l(M, m_per_chunk);
  auto dw = at::empty({N, K}, x.options().dtype(at::kFloat));
  auto part = nchunks == 1
                  ? dw
                  : at::empty({nchunks, N, K}, x.options().dtype(at::kFloat));
  dim3 grid((unsigned)std::min<long>(xy_blocks, 4096), nchunks);
  DISPATCH_16(x, T16, {
    hipLaunchKernelGGL(linear_wgrad_kernel<T16>, grid, dim3(256), 0,
                       cur_stream(), (const T16*)x.data_ptr(),
                       (const T16*)dy.data_ptr(), part.data_ptr<float>(), M,
                       N, K, m_per_chunk);
  });
  if (nchunks > 1) fold_rows(part, dw, total, nchunks);
  return dw;
}
