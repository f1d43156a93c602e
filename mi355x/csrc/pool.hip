// NHWC pooling kernels: maxpool fwd (+argmax indices),
// maxpool bwd, and global average pool.
//
// Argmax indices are stored as the RELATIVE window position r*kw+s in ONE
// byte (torch stores absolute int32 indices — 4x the traffic), and the
// backward is a GATHER: each dx element scans the <=ceil(k/stride)^2
// windows that could have picked it and sums matching dy. No fp32 scratch
// buffer, no zero-init pass, no atomics, no final cast (the old scatter
// variant measured 1.18 ms on the ResNet-50 stem pool; the gather floor
// is ~80 us of pure streaming).
#include "common.h"

namespace {

// Does tap value f replace the running maximum? The first in-image tap
// always does (no sentinel: an all -inf window gives -inf, and idx always
// names an in-image tap); after it a larger value does, the first of equal
// values stays, and a NaN wins and then sticks (!(f <= best) is true for a
// NaN f, best == best false for a NaN best), as in torch.max_pool2d: a
// forward NaN has to reach the gradient, where the loss scaler looks.
DEV_INLINE bool pool_takes(bool first, float f, float best) {
  return first || (!(f <= best) && best == best);
}

// C%8 fast path: one thread owns 8 channels of one output; window taps
// are short8 loads (16B), argmax kept per sub-lane, indices stored as one
// 8-byte pack. 8x fewer memory instructions than the scalar variant
// (PMC: scalar version sat at 77% WAIT_ANY on 2B accesses).
template <typename T16>
__global__ void maxpool_fwd_vec8(const T16* __restrict__ x,
                                 T16* __restrict__ y,
                                 unsigned char* __restrict__ idx, int N,
                                 int H, int W, int C, int P, int Q, int kh,
                                 int kw, int stride, int pad) {
  const long total = (long)N * P * Q * (C / 8);
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (long)gridDim.x * blockDim.x) {
    const int c8 = (int)(t % (C / 8));
    long npq = t / (C / 8);
    const int q = (int)(npq % Q);
    long np = npq / Q;
    const int p = (int)(np % P);
    const int n = (int)(np / P);
    float best[8] = {};
    int rs[8] = {};
    bool first = true;  // no in-image tap seen yet (pad <= k/2: there is one)
    for (int r = 0; r < kh; ++r) {
      const int ih = p * stride - pad + r;
      if (ih < 0 || ih >= H) continue;
      for (int sx = 0; sx < kw; ++sx) {
        const int iw = q * stride - pad + sx;
        if (iw < 0 || iw >= W) continue;
        const short8 v = *reinterpret_cast<const short8*>(
            x + (((long)n * H + ih) * W + iw) * C + c8 * 8);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const float f = s16_to_f32<T16>(v[u]);
          if (pool_takes(first, f, best[u])) {
            best[u] = f;
            rs[u] = r * kw + sx;
          }
        }
        first = false;
      }
    }
    short8 yv;
    unsigned char iv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      T16 h = F16<T16>::from_f32(best[u]);
      short hs;
      __builtin_memcpy(&hs, &h, 2);
      yv[u] = hs;
      iv[u] = (unsigned char)rs[u];
    }
    const long o = ((((long)n * P + p) * Q + q) * C + c8 * 8);
    *reinterpret_cast<short8*>(y + o) = yv;
    __builtin_memcpy(idx + o, iv, 8);
  }
}

template <typename T16>
__global__ void maxpool_fwd_kernel(const T16* __restrict__ x,
                                   T16* __restrict__ y,
                                   unsigned char* __restrict__ idx, int N, int H, int W,
                                   int C, int P, int Q, int kh, int kw,
                                   int stride, int pad) {
  const long total = (long)N * P * Q * C;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (long)gridDim.x * blockDim.x) {
    const int c = (int)(t % C);
    long npq = t / C;
    const int q = (int)(npq % Q);
    long np = npq / Q;
    const int p = (int)(np % P);
    const int n = (int)(np / P);
    float best = 0.f;
    int best_rs = 0;
    bool first = true;
    for (int r = 0; r < kh; ++r) {
      const int ih = p * stride - pad + r;
      if (ih < 0 || ih >= H) continue;
      for (int s = 0; s < kw; ++s) {
        const int iw = q * stride - pad + s;
        if (iw < 0 || iw >= W) continue;
        const float v =
            F16<T16>::to_f32(x[(((long)n * H + ih) * W + iw) * C + c]);
        if (pool_takes(first, v, best)) {
          best = v;
          best_rs = r * kw + s;
        }
        first = false;
      }
    }
    y[t] = F16<T16>::from_f32(best);
    idx[t] = (unsigned char)best_rs;
  }
}

// C%8 fast path of the gather backward
template <typename T16>
__global__ void maxpool_bwd_vec8(const T16* __restrict__ dy,
                                 const unsigned char* __restrict__ idx,
                                 T16* __restrict__ dx, int N, int H, int W,
                                 int C, int P, int Q, int kh, int kw,
                                 int stride, int pad) {
  const long total = (long)N * H * W * (C / 8);
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (long)gridDim.x * blockDim.x) {
    const int c8 = (int)(t % (C / 8));
    long nhw = t / (C / 8);
    const int iw = (int)(nhw % W);
    long nh = nhw / W;
    const int ih = (int)(nh % H);
    const int n = (int)(nh / H);
    const int p1 = min(P - 1, (ih + pad) / stride);
    const int p0 = max(0, (ih + pad - kh + stride) / stride);
    const int q1 = min(Q - 1, (iw + pad) / stride);
    const int q0 = max(0, (iw + pad - kw + stride) / stride);
    float acc[8] = {};
    for (int p = p0; p <= p1; ++p) {
      const int r = ih - (p * stride - pad);
      for (int q = q0; q <= q1; ++q) {
        const int sx = iw - (q * stride - pad);
        const long o = (((long)n * P + p) * Q + q) * C + c8 * 8;
        unsigned char iv[8];
        __builtin_memcpy(iv, idx + o, 8);
        const short8 dv = *reinterpret_cast<const short8*>(dy + o);
        const unsigned char want = (unsigned char)(r * kw + sx);
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (iv[u] == want) acc[u] += s16_to_f32<T16>(dv[u]);
      }
    }
    short8 ov;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      T16 h = F16<T16>::from_f32(acc[u]);
      short hs;
      __builtin_memcpy(&hs, &h, 2);
      ov[u] = hs;
    }
    *reinterpret_cast<short8*>(
        dx + ((((long)n * H + ih) * W + iw) * C + c8 * 8)) = ov;
  }
}

// gather backward: dx[n,ih,iw,c] = sum over candidate windows (p,q) of
// dy[n,p,q,c] where the stored relative argmax points back at (ih,iw)
template <typename T16>
__global__ void maxpool_bwd_kernel(const T16* __restrict__ dy,
                                   const unsigned char* __restrict__ idx,
                                   T16* __restrict__ dx, int N, int H, int W,
                                   int C, int P, int Q, int kh, int kw,
                                   int stride, int pad) {
  const long total = (long)N * H * W * C;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (long)gridDim.x * blockDim.x) {
    const int c = (int)(t % C);
    long nhw = t / C;
    const int iw = (int)(nhw % W);
    long nh = nhw / W;
    const int ih = (int)(nh % H);
    const int n = (int)(nh / H);
    // windows (p,q) with p*stride-pad <= ih <= p*stride-pad+kh-1
    const int p1 = min(P - 1, (ih + pad) / stride);
    const int p0 = max(0, (ih + pad - kh + stride) / stride);
    const int q1 = min(Q - 1, (iw + pad) / stride);
    const int q0 = max(0, (iw + pad - kw + stride) / stride);
    float acc = 0.f;
    for (int p = p0; p <= p1; ++p) {
      const int r = ih - (p * stride - pad);
      for (int q = q0; q <= q1; ++q) {
        const int s = iw - (q * stride - pad);
        const long o = (((long)n * P + p) * Q + q) * C + c;
        if (idx[o] == r * kw + s) acc += F16<T16>::to_f32(dy[o]);
      }
    }
    dx[t] = F16<T16>::from_f32(acc);
  }
}

template <typename T16>
__global__ void gap_kernel(const T16* __restrict__ x, T16* __restrict__ y,
                           int N, long HW, int C) {
  const long total = (long)N * C;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (long)gridDim.x * blockDim.x) {
    const int c = (int)(t % C);
    const int n = (int)(t / C);
    const T16* xp = x + (long)n * HW * C + c;
    float s = 0.f;
    for (long m = 0; m < HW; ++m) s += F16<T16>::to_f32(xp[m * C]);
    y[t] = F16<T16>::from_f32(s / (float)HW);
  }
}

// 16k blocks (4M threads): the bwd gather is latency-bound (PMC: 33%
// issue-stall, 49% parked at the 4096 cap) — more resident waves per
// element-iteration hide more of the 2-4 window round trips
inline int pgrid(long n) { return (int)std::min<long>(cdiv_l(n, 256), 16384); }

}  // namespace

at::Tensor cast_to_16(at::Tensor src, at::Tensor like);  // elementwise.hip

std::vector<at::Tensor> maxpool_fwd(at::Tensor x, long kernel, long stride,
                                    long pad) {
  CHECK_GPU(x);
  CHECK_CONTIG(x);
  CHECK_16BIT(x);
  // relative argmax is one byte (r*kw+s) — larger windows would alias
  TORCH_CHECK(kernel * kernel <= 256, "maxpool window ", kernel, "x", kernel,
              " exceeds the byte-packed argmax range (kernel^2 must be <=256)");
  // a window must hold an in-image tap (torch's rule too): with more
  // padding the output would be a maximum over nothing
  TORCH_CHECK(pad >= 0 && pad <= kernel / 2, "maxpool pad ", pad,
              " must be at most half the kernel size ", kernel);
  const int N = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  const int P = (H + 2 * pad - kernel) / stride + 1;
  const int Q = (W + 2 * pad - kernel) / stride + 1;
  auto y = at::empty({N, P, Q, C}, x.options());
  auto idx = at::empty({N, P, Q, C}, x.options().dtype(at::kByte));
  DISPATCH_16(x, T16, {
    if (C % 8 == 0)
      hipLaunchKernelGGL(maxpool_fwd_vec8<T16>,
                         dim3(pgrid((long)N * P * Q * (C / 8))), dim3(256), 0,
                         cur_stream(), (const T16*)x.data_ptr(),
                         (T16*)y.data_ptr(), idx.data_ptr<unsigned char>(), N,
                         H, W, C, P, Q, (int)kernel, (int)kernel, (int)stride,
                         (int)pad);
    else
      hipLaunchKernelGGL(maxpool_fwd_kernel<T16>,
                         dim3(pgrid((long)N * P * Q * C)), dim3(256), 0,
                         cur_stream(), (const T16*)x.data_ptr(),
                         (T16*)y.data_ptr(), idx.data_ptr<unsigned char>(), N,
                         H, W, C, P, Q, (int)kernel, (int)kernel, (int)stride,
                         (int)pad);
  });
  return {y, idx};
}

at::Tensor maxpool_bwd(at::Tensor dy, at::Tensor idx, long H, long W,
                       long kernel, long stride, long pad) {
  CHECK_GPU(dy);
  CHECK_CONTIG(dy);
  TORCH_CHECK(kernel * kernel <= 256, "maxpool window ", kernel, "x", kernel,
              " exceeds the byte-packed argmax range (kernel^2 must be <=256)");
  // a window must hold an in-image tap (torch's rule too): with more
  // padding the output would be a maximum over nothing
  TORCH_CHECK(pad >= 0 && pad <= kernel / 2, "maxpool pad ", pad,
              " must be at most half the kernel size ", kernel);
  const int N = dy.size(0), P = dy.size(1), Q = dy.size(2), C = dy.size(3);
  auto dx = at::empty({N, H, W, (long)C}, dy.options());
  DISPATCH_16(dy, T16, {
    if (C % 8 == 0)
      hipLaunchKernelGGL(maxpool_bwd_vec8<T16>,
                         dim3(pgrid((long)N * H * W * (C / 8))), dim3(256), 0,
                         cur_stream(), (const T16*)dy.data_ptr(),
                         idx.data_ptr<unsigned char>(), (T16*)dx.data_ptr(),
                         N, (int)H, (int)W, C, P, Q, (int)kernel, (int)kernel,
                         (int)stride, (int)pad);
    else
      hipLaunchKernelGGL(maxpool_bwd_kernel<T16>,
                         dim3(pgrid((long)N * H * W * C)), dim3(256), 0,
                         cur_stream(), (const T16*)dy.data_ptr(),
                         idx.data_ptr<unsigned char>(), (T16*)dx.data_ptr(),
                         N, (int)H, (int)W, C, P, Q, (int)kernel, (int)kernel,
                         (int)stride, (int)pad);
  });
  return dx;
}

at::Tensor global_avg_pool(at::Tensor x) {
  CHECK_GPU(x);
  CHECK_CONTIG(x);
  CHECK_16BIT(x);
  const int N = x.size(0), C = x.size(3);
  const long HW = (long)x.size(1) * x.size(2);
  auto y = at::empty({N, C}, x.options());
  DISPATCH_16(x, T16, {
    hipLaunchKernelGGL(gap_kernel<T16>, dim3(pgrid((long)N * C)), dim3(256),
                       0, cur_stream(), (const T16*)x.data_ptr(),
                       (T16*)y.data_ptr(), N, HW, C);
  });
  return y;
}
