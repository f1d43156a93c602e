// Squeeze-and-Excitation (Hu et al. 2018) over NHWC 16-bit activations with
// the block-exit residual add and ReLU fused, fp32 arithmetic:
//
//   s[n,c] = mean_hw x[n,h,w,c]
//   z[n,j] = relu(sum_c w1[j,c] s[n,c] + b1[j])              j < Cr
//   g[n,c] = sigmoid(sum_j w2[c,j] z[n,j] + b2[c])
//   y      = act(x * g[n,c] + residual)        one rounding to x's dtype
//
// The gate needs every channel of a sample, so the unit of work is a whole
// sample. A team's lanes form a grid of C/8 columns (one 16-byte channel
// octet each) by TS/(C/8) pixel rows; lane (r, c8) owns pixels r, r+rows,
// ... of its octet, so its eight channel partial sums never change
// channel. Consecutive lanes read consecutive 16-byte vectors.
//
// Resident path: a team of 64/256/1024 threads keeps its sample in
// REGISTERS (NV vectors a lane, fully unrolled) from the one HBM read to
// the store of y or dx. The channel partials fold by wave shuffles (C/8 a
// power of two below 64) and then across waves, or across pixel rows,
// through LDS in row order into s[C]; FC1, ReLU, FC2 and the sigmoid run
// out of LDS; the apply multiplies the registers. The backward holds x
// and dy together: p = dy*mask, dg = sum_hw p*x, the gate backward in LDS,
// dx = p*g + ds/HW: one read of x and dy, one write of dx (and of dres).
// Teams of 64 put four samples into a 256-thread block.
//
// Weight traffic: w1 and w2 are fp32 and, at C=512 Cr=32, eight times the
// bytes of a 4x4 sample. Both FC loops run once per BLOCK over all its
// samples: every weight is loaded once and used for each of them (4 in a
// resident block of 64-thread teams, 16 in the streamed gate kernels).
// w2 arrives transposed ([Cr,C]) so that every weight read is coalesced.
//
// Streamed path (samples that do not fit): a chunk kernel per (sample,
// pixel-chunk) writes partial channel sums, a gate kernel per 16 samples (4
// above 512 channels) adds them in chunk order and produces s, z, g, an
// elementwise kernel applies.
// Backward: chunk sums of p*x, the gate backward, an elementwise dx.
//
// Path rule (measured, profiles/r15_se.md): resident wherever a team can
// hold the sample, in both directions: at most 16 vectors a lane in a team
// of 64, 8 in a team of 256 or 1024, the smallest team that fits (128 KiB
// of x at 64 channels; se_res_cfg). It beat the streamed path at all four
// ResNet-18 shapes at batch 8192, forward by 1.26x to 1.5x and forward +
// backward by 1.08x to 1.29x, so the streamed path serves only samples
// that do not fit (56x56x256, 48x48x64).
//
// Parameter gradients come from the fp32 side outputs (s, z, dl, dz) in
// se_wgrad: N is split, every split writes one row, fold_rows adds them.
//
// Every reduction has a fixed order; no float atomics; two runs give the
// same bits. Activation offsets are 64-bit, index decomposition is 32-bit.
// An absent tensor arrives as an empty tensor's pointer plus a flag bit; a
// kernel never tests a pointer.
#include "common.h"

// no packed-fp32 instructions in this file (see gn.hip)
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

constexpr int kMaxC = 2048, kMaxCr = 256;
constexpr int kSPerBlock = 2048;  // LDS floats for s/g of a resident block

struct SEDims {
  int N, HW, C, Cr;
  int cv;  // 16-byte vectors per pixel: C / 8
};

enum : int { kRelu = 1, kHasRes = 2, kSide = 4, kMask = 8 };

// Per-channel totals of a team of TS threads. q[u]: the lane's partial for
// channel c8*8 + u (zero on idle lanes). `red` is the team's TS*8 floats.
// Out: tot[c], c < C, rows added in order. Every thread of the block calls
// this (it synchronises the block).
template <int TS>
DEV_INLINE void team_fold(float (&q)[8], float* red, float* tot,
                          const SEDims& d, int t, int r, int c8, int rows) {
  const bool shfl = d.cv < 64 && (d.cv & (d.cv - 1)) == 0;
  int row = r, nrows = rows;
  bool writer = r < rows;
  if (shfl) {  // lanes of a wave that share an octet are cv apart
    for (int off = 32; off >= d.cv; off >>= 1) {
#pragma unroll
      for (int u = 0; u < 8; ++u) q[u] += __shfl_xor(q[u], off, kWave);
    }
    row = t >> 6;
    nrows = TS / 64;
    writer = (t & 63) < d.cv;
  }
  __syncthreads();  // readers of the previous call's red/tot are done
  if (writer) {
#pragma unroll
    for (int u = 0; u < 8; ++u) red[row * d.C + c8 * 8 + u] = q[u];
  }
  __syncthreads();
  for (int c = t; c < d.C; c += TS) {
    // four interleaved partial sums, then pairwise: a quarter of the
    // dependent adds and of the rounding steps a value goes through
    float a[4] = {};
    int k = 0;
    for (; k + 4 <= nrows; k += 4) {
#pragma unroll
      for (int m = 0; m < 4; ++m) a[m] += red[(k + m) * d.C + c];
    }
#pragma unroll
    for (int m = 0; m < 3; ++m)
      if (k + m < nrows) a[m] += red[(k + m) * d.C + c];
    tot[c] = (a[0] + a[1]) + (a[2] + a[3]);
  }
  __syncthreads();
}

DEV_INLINE float wave_sum(float a) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) a += __shfl_xor(a, off, kWave);
  return a;
}

DEV_INLINE float sigmoid_f(float l) {
  // exp overflows to +inf for l < -88: 1 / inf = 0, never inf / inf
  return 1.f / (1.f + expf(-l));
}

// The gate of SPB samples n0 .. n0+SPB-1 by a block of T threads: every
// weight is read once for all of them. sg: [SPB][C] in LDS, s on entry
// (already synchronised), g on return. zl: [SPB][Cr] in LDS.
template <int SPB, int T>
DEV_INLINE void gate_fwd(float* sg, float* zl, const float* __restrict__ w1,
                         const float* __restrict__ b1,
                         const float* __restrict__ w2t,
                         const float* __restrict__ b2, float* z_out,
                         float* g_out, int wz, int wg, const SEDims& d,
                         int n0) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int j = w; j < d.Cr; j += T / 64) {
    float acc[SPB] = {};
    for (int c = lane; c < d.C; c += 64) {
      const float wv = w1[j * d.C + c];
#pragma unroll
      for (int k = 0; k < SPB; ++k) acc[k] += wv * sg[k * d.C + c];
    }
#pragma unroll
    for (int k = 0; k < SPB; ++k) acc[k] = wave_sum(acc[k]);
    if (lane == 0) {
      const float b = b1[j];
#pragma unroll
      for (int k = 0; k < SPB; ++k) {
        const float zz = relu_f(acc[k] + b);
        zl[k * d.Cr + j] = zz;
        if (wz && n0 + k < d.N) z_out[(long)(n0 + k) * d.Cr + j] = zz;
      }
    }
  }
  __syncthreads();  // z complete, s no longer read
  for (int c = threadIdx.x; c < d.C; c += T) {
    float acc[SPB];
    const float b = b2[c];
#pragma unroll
    for (int k = 0; k < SPB; ++k) acc[k] = b;
    for (int j = 0; j < d.Cr; ++j) {
      const float wv = w2t[j * d.C + c];
#pragma unroll
      for (int k = 0; k < SPB; ++k) acc[k] += wv * zl[k * d.Cr + j];
    }
#pragma unroll
    for (int k = 0; k < SPB; ++k) {
      const float gg = sigmoid_f(acc[k]);
      sg[k * d.C + c] = gg;
      if (wg && n0 + k < d.N) g_out[(long)(n0 + k) * d.C + c] = gg;
    }
  }
  __syncthreads();
}

// The gate backward of SPB samples. dgl: [SPB][C] in LDS, dg on entry
// (synchronised), dl after the first step, ds / HW on return. dl and dz
// also go out in fp32 for the parameter gradients.
template <int SPB, int T>
DEV_INLINE void gate_bwd(float* dgl, float* dzl,
                         const float* __restrict__ g,
                         const float* __restrict__ z,
                         const float* __restrict__ w1,
                         const float* __restrict__ w2t, float* dl_out,
                         float* dz_out, const SEDims& d, int n0) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int c = threadIdx.x; c < d.C; c += T) {
#pragma unroll
    for (int k = 0; k < SPB; ++k) {
      float v = 0.f;
      if (n0 + k < d.N) {
        const float gg = g[(long)(n0 + k) * d.C + c];
        v = dgl[k * d.C + c] * gg * (1.f - gg);
        dl_out[(long)(n0 + k) * d.C + c] = v;
      }
      dgl[k * d.C + c] = v;
    }
  }
  __syncthreads();
  for (int j = w; j < d.Cr; j += T / 64) {
    float acc[SPB] = {};
    for (int c = lane; c < d.C; c += 64) {
      const float wv = w2t[j * d.C + c];
#pragma unroll
      for (int k = 0; k < SPB; ++k) acc[k] += wv * dgl[k * d.C + c];
    }
#pragma unroll
    for (int k = 0; k < SPB; ++k) acc[k] = wave_sum(acc[k]);
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < SPB; ++k) {
        float v = 0.f;
        if (n0 + k < d.N) {
          v = z[(long)(n0 + k) * d.Cr + j] > 0.f ? acc[k] : 0.f;
          dz_out[(long)(n0 + k) * d.Cr + j] = v;
        }
        dzl[k * d.Cr + j] = v;
      }
    }
  }
  __syncthreads();
  const float hw = (float)d.HW;
  for (int c = threadIdx.x; c < d.C; c += T) {
    float acc[SPB] = {};
    for (int j = 0; j < d.Cr; ++j) {
      const float wv = w1[j * d.C + c];
#pragma unroll
      for (int k = 0; k < SPB; ++k) acc[k] += wv * dzl[k * d.Cr + j];
    }
#pragma unroll
    for (int k = 0; k < SPB; ++k) dgl[k * d.C + c] = acc[k] / hw;
  }
  __syncthreads();
}

// ---- resident path ---------------------------------------------------------

#define SE_TEAM_SETUP                                                     \
  constexpr int T = TS < 256 ? 256 : TS;                                  \
  constexpr int TPB = T / TS; /* samples per block */                     \
  __shared__ float red[T * 8];                                            \
  const int team = threadIdx.x / TS, t = threadIdx.x % TS;                \
  const int n0 = blockIdx.x * TPB;                                        \
  const bool on = n0 + team < d.N; /* a team past the end idles */        \
  const int n = on ? n0 + team : 0;                                       \
  const int rows = TS / d.cv;     /* pixel rows of the lane grid */       \
  const int r = t / d.cv, c8 = t - r * d.cv;                              \
  const bool live = on && r < rows;                                       \
  const long base = (long)n * d.HW * d.C + c8 * 8

template <typename T16, int TS, int NV>
__global__ __launch_bounds__(TS < 256 ? 256 : TS) void se_fwd_res(
    const T16* __restrict__ x, const float* __restrict__ w1,
    const float* __restrict__ b1, const float* __restrict__ w2t,
    const float* __restrict__ b2, const T16* __restrict__ res,
    T16* __restrict__ y, unsigned char* __restrict__ msk,
    float* __restrict__ s_out, float* __restrict__ z_out,
    float* __restrict__ g_out, SEDims d, int flags) {
  SE_TEAM_SETUP;
  __shared__ float sg[kSPerBlock];
  __shared__ float zl[TPB * kMaxCr];
  short8 xv[NV];
  float q[8] = {};
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int p = r + i * rows;
    xv[i] = short8{};
    if (live && p < d.HW)
      xv[i] = *reinterpret_cast<const short8*>(x + base + (long)p * d.C);
  }
#pragma unroll
  for (int i = 0; i < NV; ++i)  // vectors past HW hold zeros
#pragma unroll
    for (int u = 0; u < 8; ++u) q[u] += s16_to_f32<T16>(xv[i][u]);
  // keep the sample packed across the gate (no fp32 copies carried over)
#pragma unroll
  for (int i = 0; i < NV; ++i) asm volatile("" : "+v"(xv[i]));
  float* st = sg + team * d.C;
  team_fold<TS>(q, red + team * TS * 8, st, d, t, r, c8, rows);
  const float hw = (float)d.HW;
  for (int c = t; c < d.C; c += TS) {  // a thread's own channels of tot
    const float m = st[c] / hw;
    st[c] = m;
    if ((flags & kSide) && on) s_out[(long)n * d.C + c] = m;
  }
  __syncthreads();
  gate_fwd<TPB, T>(sg, zl, w1, b1, w2t, b2, z_out, g_out, flags & kSide,
                   flags & kSide, d, n0);
  float gl[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) gl[u] = live ? st[c8 * 8 + u] : 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int p = r + i * rows;
    if (live && p < d.HW) {
      const long e = base + (long)p * d.C;
      short8 vr = {};
      if (flags & kHasRes) vr = *reinterpret_cast<const short8*>(res + e);
      short8 o;
      unsigned mb = 0;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        float v = s16_to_f32<T16>(xv[i][u]) * gl[u];
        if (flags & kHasRes) v += s16_to_f32<T16>(vr[u]);
        if (flags & kRelu) v = relu_f(v);
        o[u] = f32_to_s16<T16>(v);
        if (s16_to_f32<T16>(o[u]) > 0.f) mb |= 1u << u;
      }
      *reinterpret_cast<short8*>(y + e) = o;
      if (flags & kMask) msk[e >> 3] = (unsigned char)mb;
    }
  }
}

template <typename T16, int TS, int NV>
__global__ __launch_bounds__(TS < 256 ? 256 : TS) void se_bwd_res(
    const T16* __restrict__ x, const T16* __restrict__ dy,
    const unsigned char* __restrict__ msk, const float* __restrict__ g,
    const float* __restrict__ z, const float* __restrict__ w1,
    const float* __restrict__ w2t, T16* __restrict__ dx,
    T16* __restrict__ dres, float* __restrict__ dl_out,
    float* __restrict__ dz_out, SEDims d, int flags) {
  SE_TEAM_SETUP;
  __shared__ float dgl[kSPerBlock];  // dg, then dl, then ds / HW
  __shared__ float dzl[TPB * kMaxCr];
  short8 xv[NV], dv[NV];  // dv holds the masked dy from here on
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int p = r + i * rows;
    xv[i] = short8{};
    dv[i] = short8{};
    if (live && p < d.HW) {
      const long e = base + (long)p * d.C;
      xv[i] = *reinterpret_cast<const short8*>(x + e);
      dv[i] = *reinterpret_cast<const short8*>(dy + e);
      if (flags & kMask) {
        const unsigned mb = msk[e >> 3];
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (!((mb >> u) & 1)) dv[i][u] = 0;
      }
    }
  }
  float q[8] = {};
#pragma unroll
  for (int i = 0; i < NV; ++i)  // vectors past HW hold zeros
#pragma unroll
    for (int u = 0; u < 8; ++u)
      q[u] += s16_to_f32<T16>(dv[i][u]) * s16_to_f32<T16>(xv[i][u]);
  // keep the sample packed across the gate (as gn_bwd_res does)
#pragma unroll
  for (int i = 0; i < NV; ++i) asm volatile("" : "+v"(xv[i]), "+v"(dv[i]));
  team_fold<TS>(q, red + team * TS * 8, dgl + team * d.C, d, t, r, c8, rows);
  gate_bwd<TPB, T>(dgl, dzl, g, z, w1, w2t, dl_out, dz_out, d, n0);
  float gl[8], ds[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    gl[u] = live ? g[(long)n * d.C + c8 * 8 + u] : 0.f;
    ds[u] = live ? dgl[team * d.C + c8 * 8 + u] : 0.f;
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int p = r + i * rows;
    if (live && p < d.HW) {
      const long e = base + (long)p * d.C;
      short8 o;
#pragma unroll
      for (int u = 0; u < 8; ++u)
        o[u] = f32_to_s16<T16>(s16_to_f32<T16>(dv[i][u]) * gl[u] + ds[u]);
      *reinterpret_cast<short8*>(dx + e) = o;
      if (flags & kHasRes) *reinterpret_cast<short8*>(dres + e) = dv[i];
    }
  }
}

// ---- streamed path ---------------------------------------------------------

constexpr int kChunkVec = 2048;  // vectors of a default chunk: 8 per lane

// one (sample, pixel-chunk) per block: per-channel sums of x (forward) or
// of p*x (BWD) over the chunk into part[N][nchunks][C]
template <typename T16, bool BWD>
__global__ __launch_bounds__(256) void se_sum_chunk(
    const T16* __restrict__ x, const T16* __restrict__ dy,
    const unsigned char* __restrict__ msk, float* __restrict__ part,
    SEDims d, int nchunks, int chunk_px, int flags) {
  __shared__ float red[256 * 8];
  __shared__ float tot[kMaxC];
  const int t = threadIdx.x;
  const int n = blockIdx.x / nchunks, ch = blockIdx.x - n * nchunks;
  const int rows = 256 / d.cv;
  const int r = t / d.cv, c8 = t - r * d.cv;
  const int p0 = ch * chunk_px, np = min(chunk_px, d.HW - p0);
  const long base = ((long)n * d.HW + p0) * d.C + c8 * 8;
  float q[8] = {};
  if (r < rows) {
#pragma unroll 4
    for (int p = r; p < np; p += rows) {
      const long e = base + (long)p * d.C;
      const short8 vx = *reinterpret_cast<const short8*>(x + e);
      if (BWD) {
        const short8 vd = *reinterpret_cast<const short8*>(dy + e);
        const unsigned mb = (flags & kMask) ? msk[e >> 3] : 0xffu;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const float dd = ((mb >> u) & 1) ? s16_to_f32<T16>(vd[u]) : 0.f;
          q[u] += dd * s16_to_f32<T16>(vx[u]);
        }
      } else {
#pragma unroll
        for (int u = 0; u < 8; ++u) q[u] += s16_to_f32<T16>(vx[u]);
      }
    }
  }
  team_fold<256>(q, red, tot, d, t, r, c8, rows);
  float* o = part + ((long)n * nchunks + ch) * d.C;
  for (int c = t; c < d.C; c += 256) o[c] = tot[c];
}

// SPB samples per block: the chunk rows added in order, then the gate
template <int SPB>
__global__ __launch_bounds__(256) void se_gate_fwd_str(
    const float* __restrict__ part, const float* __restrict__ w1,
    const float* __restrict__ b1, const float* __restrict__ w2t,
    const float* __restrict__ b2, float* __restrict__ s_out,
    float* __restrict__ z_out, float* __restrict__ g_out, SEDims d,
    int nchunks, int flags) {
  __shared__ float sg[SPB * (8192 / SPB)];  // SPB 16: C <= 512; 4: 2048
  __shared__ float zl[SPB * kMaxCr];
  const int n0 = blockIdx.x * SPB;
  const float hw = (float)d.HW;
  for (int k = 0; k < SPB; ++k) {
    const int n = n0 + k;
    for (int c = threadIdx.x; c < d.C; c += 256) {
      float a = 0.f;
      if (n < d.N) {
        const float* p = part + (long)n * nchunks * d.C + c;
        for (int ch = 0; ch < nchunks; ++ch) a += p[(long)ch * d.C];
        a = a / hw;
        if (flags & kSide) s_out[(long)n * d.C + c] = a;
      }
      sg[k * d.C + c] = a;
    }
  }
  __syncthreads();
  gate_fwd<SPB, 256>(sg, zl, w1, b1, w2t, b2, z_out, g_out, flags & kSide, 1,
                     d, n0);
}

template <int SPB>
__global__ __launch_bounds__(256) void se_gate_bwd_str(
    const float* __restrict__ part, const float* __restrict__ g,
    const float* __restrict__ z, const float* __restrict__ w1,
    const float* __restrict__ w2t, float* __restrict__ dl_out,
    float* __restrict__ dz_out, float* __restrict__ ds_out, SEDims d,
    int nchunks) {
  __shared__ float dgl[SPB * (8192 / SPB)];  // dg, then dl, then ds / HW
  __shared__ float dzl[SPB * kMaxCr];
  const int n0 = blockIdx.x * SPB;
  for (int k = 0; k < SPB; ++k) {
    const int n = n0 + k;
    for (int c = threadIdx.x; c < d.C; c += 256) {
      float a = 0.f;
      if (n < d.N) {
        const float* p = part + (long)n * nchunks * d.C + c;
        for (int ch = 0; ch < nchunks; ++ch) a += p[(long)ch * d.C];
      }
      dgl[k * d.C + c] = a;
    }
  }
  __syncthreads();
  gate_bwd<SPB, 256>(dgl, dzl, g, z, w1, w2t, dl_out, dz_out, d, n0);
  for (int k = 0; k < SPB; ++k) {
    const int n = n0 + k;
    if (n < d.N)
      for (int c = threadIdx.x; c < d.C; c += 256)
        ds_out[(long)n * d.C + c] = dgl[k * d.C + c];
  }
}

// elementwise sweep of one sample per block row: blockIdx.x = n*bps + b.
// A thread's channel octet is the same for all its vectors when `inv`
// (its stride is a multiple of C/8): the gate is loaded once.
#define SE_SWEEP_SETUP                                                    \
  const int n = blockIdx.x / bps, b = blockIdx.x - n * bps;               \
  const int VS = d.HW * d.cv; /* vectors per sample */                    \
  const long sbase = (long)n * d.HW * d.C;                                \
  const int stride = bps * 256;                                           \
  int v = b * 256 + threadIdx.x

template <typename T16>
__global__ __launch_bounds__(256) void se_apply_str(
    const T16* __restrict__ x, const float* __restrict__ g,
    const T16* __restrict__ res, T16* __restrict__ y,
    unsigned char* __restrict__ msk, SEDims d, int bps, int inv, int flags) {
  SE_SWEEP_SETUP;
  float gl[8];
  auto params = [&](int c0) {
#pragma unroll
    for (int u = 0; u < 8; ++u) gl[u] = g[(long)n * d.C + c0 + u];
  };
  if (inv && v < VS) params((v % d.cv) * 8);
  for (; v < VS; v += stride) {
    if (!inv) params((v % d.cv) * 8);
    const long e = sbase + (long)v * 8;
    const short8 vx = *reinterpret_cast<const short8*>(x + e);
    short8 vr = {};
    if (flags & kHasRes) vr = *reinterpret_cast<const short8*>(res + e);
    short8 o;
    unsigned mb = 0;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      float r = s16_to_f32<T16>(vx[u]) * gl[u];
      if (flags & kHasRes) r += s16_to_f32<T16>(vr[u]);
      if (flags & kRelu) r = relu_f(r);
      o[u] = f32_to_s16<T16>(r);
      if (s16_to_f32<T16>(o[u]) > 0.f) mb |= 1u << u;
    }
    *reinterpret_cast<short8*>(y + e) = o;
    if (flags & kMask) msk[e >> 3] = (unsigned char)mb;
  }
}

template <typename T16>
__global__ __launch_bounds__(256) void se_bwd_dx_str(
    const T16* __restrict__ x, const T16* __restrict__ dy,
    const unsigned char* __restrict__ msk, const float* __restrict__ g,
    const float* __restrict__ ds, T16* __restrict__ dx,
    T16* __restrict__ dres, SEDims d, int bps, int inv, int flags) {
  SE_SWEEP_SETUP;
  float gl[8], dl[8];
  auto params = [&](int c0) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      gl[u] = g[(long)n * d.C + c0 + u];
      dl[u] = ds[(long)n * d.C + c0 + u];
    }
  };
  if (inv && v < VS) params((v % d.cv) * 8);
  for (; v < VS; v += stride) {
    if (!inv) params((v % d.cv) * 8);
    const long e = sbase + (long)v * 8;
    short8 vd = *reinterpret_cast<const short8*>(dy + e);
    const unsigned mb = (flags & kMask) ? msk[e >> 3] : 0xffu;
    short8 o;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (!((mb >> u) & 1)) vd[u] = 0;
      o[u] = f32_to_s16<T16>(s16_to_f32<T16>(vd[u]) * gl[u] + dl[u]);
    }
    *reinterpret_cast<short8*>(dx + e) = o;
    if (flags & kHasRes) *reinterpret_cast<short8*>(dres + e) = vd;
  }
}

// ---- parameter gradients ---------------------------------------------------

// Block (cx, jy, zc): 64 channels x 4*JPT hidden units over split zc of N.
// A thread owns channel c and JPT hidden units (the same for its wave):
// dw1[j,c] += dz[n,j] s[n,c], dw2[c,j] += dl[n,c] z[n,j], n in order.
// Row zc of part is [dw1 (Cr*C) | db1 (Cr) | dw2 (C*Cr) | db2 (C)].
template <int JPT>
__global__ __launch_bounds__(256) void se_wgrad_part(
    const float* __restrict__ s, const float* __restrict__ z,
    const float* __restrict__ dl, const float* __restrict__ dz,
    float* __restrict__ part, SEDims d, int nper, long E) {
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const int j0 = blockIdx.y * (4 * JPT) + (threadIdx.x >> 6) * JPT;
  const int na = blockIdx.z * nper, nb = min(d.N, na + nper);
  const bool cok = c < d.C;
  float a1[JPT] = {}, a2[JPT] = {}, ab1[JPT] = {}, ab2 = 0.f;
  for (int n = na; n < nb; ++n) {
    const float dlv = cok ? dl[(long)n * d.C + c] : 0.f;
    const float sv = cok ? s[(long)n * d.C + c] : 0.f;
    ab2 += dlv;
#pragma unroll
    for (int u = 0; u < JPT; ++u) {
      if (j0 + u < d.Cr) {
        const float zv = z[(long)n * d.Cr + j0 + u];
        const float dzv = dz[(long)n * d.Cr + j0 + u];
        a1[u] += dzv * sv;
        a2[u] += dlv * zv;
        ab1[u] += dzv;
      }
    }
  }
  float* o = part + (long)blockIdx.z * E;
  const long o_b1 = (long)d.Cr * d.C, o_w2 = o_b1 + d.Cr,
             o_b2 = o_w2 + (long)d.C * d.Cr;
#pragma unroll
  for (int u = 0; u < JPT; ++u) {
    const int j = j0 + u;
    if (j < d.Cr) {
      if (cok) {
        o[(long)j * d.C + c] = a1[u];
        o[o_w2 + (long)c * d.Cr + j] = a2[u];
      }
      if (blockIdx.x == 0 && (threadIdx.x & 63) == 0) o[o_b1 + j] = ab1[u];
    }
  }
  if (cok && blockIdx.y == 0 && (threadIdx.x >> 6) == 0) o[o_b2 + c] = ab2;
}

#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif

// ---- host ------------------------------------------------------------------

SEDims se_dims(const at::Tensor& x, const at::Tensor& w1,
               const at::Tensor& w2t) {
  TORCH_CHECK(x.dim() == 4, "squeeze_excite: x must be NHWC [N,H,W,C]");
  const long N = x.size(0), HW = x.size(1) * x.size(2), C = x.size(3);
  TORCH_CHECK(C % 8 == 0 && C >= 8 && C <= kMaxC, "squeeze_excite: channels=",
              C, " must be a multiple of 8 in [8, ", kMaxC, "]");
  TORCH_CHECK(w1.dim() == 2 && w1.size(1) == C && w1.size(0) >= 1 &&
                  w1.size(0) <= kMaxCr,
              "squeeze_excite: w1 must be [Cr,C], Cr in [1, ", kMaxCr, "]");
  const long Cr = w1.size(0);
  TORCH_CHECK(w2t.dim() == 2 && w2t.size(0) == Cr && w2t.size(1) == C,
              "squeeze_excite: the transposed w2 must be [Cr,C]");
  TORCH_CHECK(N >= 1 && HW >= 1 && HW * C < (1L << 31) && N < (1L << 26),
              "squeeze_excite: sample or batch too large");
  for (const at::Tensor* w : {&w1, &w2t})
    TORCH_CHECK(w->is_cuda() && w->is_contiguous() &&
                    w->scalar_type() == at::kFloat,
                "squeeze_excite: weights must be contiguous fp32 on the GPU");
  return SEDims{(int)N, (int)HW, (int)C, (int)Cr, (int)(C / 8)};
}

void se_check_f32(const at::Tensor& t, long numel, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
                  t.scalar_type() == at::kFloat && t.numel() == numel,
              "squeeze_excite: ", what, " must be fp32 with ", numel,
              " elements");
}

// The most vectors a lane holds of x (and, in the backward, as many of dy
// beside them): 16 in a team of 64, 8 in the larger teams (a 1024-thread
// block has 128 VGPRs a lane).
struct MaxNV {
  int t64, t256, t1024;
};
constexpr MaxNV kFwdMaxNV{16, 8, 8}, kBwdMaxNV{16, 8, 8};

// Resident team shape as TS*100 + NV: the smallest team whose lane grid
// (C/8 columns) holds the sample within `m` vectors a lane; 0: none does.
int se_res_cfg(const SEDims& d, const MaxNV& m) {
  const int ts[3] = {64, 256, 1024}, cap[3] = {m.t64, m.t256, m.t1024};
  for (int k = 0; k < 3; ++k) {
    if (d.cv > ts[k]) continue;
    if (ts[k] == 64 && 4 * d.C > kSPerBlock) continue;  // four s rows in LDS
    const int need = cdiv_i(d.HW, ts[k] / d.cv);
    if (need > cap[k]) continue;
    int nv = 1;
    while (nv < need) nv *= 2;
    return ts[k] * 100 + nv;
  }
  return 0;
}

int se_pick_path(long path, int cfg, const char* who) {
  TORCH_CHECK(path >= 0 && path <= 2, who, ": path must be 0, 1 or 2");
  TORCH_CHECK(path != 1 || cfg != 0, who,
              ": the resident path cannot hold a sample of this shape");
  return path == 0 ? (cfg ? 1 : 2) : (int)path;
}

inline unsigned se_grid(long blocks) {
  TORCH_CHECK(blocks >= 1 && blocks < (1L << 31),
              "squeeze_excite: too many blocks");
  return (unsigned)blocks;
}

inline int se_chunk_px(const SEDims& d, long chunk, const char* who) {
  TORCH_CHECK(chunk >= 0 && chunk <= (1 << 16), who, ": chunk=", chunk,
              " must be in [0, 65536]");
  return chunk ? (int)chunk : std::max(1, kChunkVec / d.cv);
}

// elementwise sweeps: blocks per sample (about four vectors per thread),
// and whether a thread's channel octet is stride-invariant
inline int se_sweep_bps(const SEDims& d, int& inv) {
  const int bps =
      (int)std::min<long>(cdiv_l((long)d.HW * d.cv, 1024), 1 << 16);
  inv = (bps * 256) % d.cv == 0;
  return bps;
}

}  // namespace

// returns {y, s[N,C], z[N,Cr], g[N,C], mask}. want_side: the fp32 side
// outputs and (with act == relu) the 1-bit "y > 0" mask are written; else
// they come back empty. res: empty = none. w2t: w2 transposed, [Cr,C].
// path: 0 auto, 1 resident, 2 streamed; chunk: pixels per streamed chunk
// (0 auto).
std::vector<at::Tensor> se_fwd(at::Tensor x, at::Tensor w1, at::Tensor b1,
                               at::Tensor w2t, at::Tensor b2, at::Tensor res,
                               long act, bool want_side, long path,
                               long chunk) {
  CHECK_GPU(x);
  CHECK_CONTIG(x);
  CHECK_16BIT(x);
  const SEDims d = se_dims(x, w1, w2t);
  se_check_f32(b1, d.Cr, "b1");
  se_check_f32(b2, d.C, "b2");
  const bool has_res = res.numel() > 0;
  TORCH_CHECK(!has_res || (res.sizes() == x.sizes() && res.is_contiguous() &&
                           res.is_cuda() &&
                           res.scalar_type() == x.scalar_type()),
              "squeeze_excite: residual must match x");
  const int cfg = se_res_cfg(d, kFwdMaxNV);
  const int p = se_pick_path(path, cfg, "se_fwd");
  const int chunk_px = se_chunk_px(d, chunk, "se_fwd");
  const int nchunks = cdiv_i(d.HW, chunk_px);
  const bool want_mask = want_side && act == 1;
  const int flags = (act == 1 ? kRelu : 0) | (has_res ? kHasRes : 0) |
                    (want_side ? kSide : 0) | (want_mask ? kMask : 0);

  auto f32 = x.options().dtype(at::kFloat);
  auto u8 = x.options().dtype(at::kByte);
  auto y = at::empty_like(x);
  const long ns = want_side ? d.N : 0;
  auto s = at::empty({ns, d.C}, f32), z = at::empty({ns, d.Cr}, f32);
  auto g = at::empty({(want_side || p == 2) ? d.N : 0, d.C}, f32);
  auto mask = at::empty({want_mask ? x.numel() / 8 : 0}, u8);

  if (p == 1) {
    DISPATCH_16(x, T16, {
      pick<6401, 6402, 6404, 6408, 6416, 25601, 25602, 25604, 25608, 102402,
           102404, 102408>(cfg, [&](auto CFG) {
        constexpr int TS = decltype(CFG)::value / 100;
        constexpr int NV = decltype(CFG)::value % 100;
        constexpr int T = TS < 256 ? 256 : TS;
        hipLaunchKernelGGL(
            (se_fwd_res<T16, TS, NV>), dim3(se_grid(cdiv_l(d.N, T / TS))),
            dim3(T), 0, cur_stream(), (const T16*)x.data_ptr(),
            w1.data_ptr<float>(), b1.data_ptr<float>(),
            w2t.data_ptr<float>(), b2.data_ptr<float>(),
            (const T16*)res.data_ptr(), (T16*)y.data_ptr(),
            mask.data_ptr<unsigned char>(), s.data_ptr<float>(),
            z.data_ptr<float>(), g.data_ptr<float>(), d, flags);
      });
    });
    return {y, s, z, g, mask};
  }
  auto part = at::empty({d.N, nchunks, d.C}, f32);
  int inv;
  const int bps = se_sweep_bps(d, inv);
  DISPATCH_16(x, T16, {
    launch256((se_sum_chunk<T16, false>), dim3(se_grid((long)d.N * nchunks)),
              0, (const T16*)x.data_ptr(), (const T16*)x.data_ptr(),
              mask.data_ptr<unsigned char>(), part.data_ptr<float>(), d,
              nchunks, chunk_px, 0);
    pick<16, 4>(d.C <= 512 ? 16 : 4, [&](auto SPB) {
      launch256(se_gate_fwd_str<decltype(SPB)::value>,
                dim3(se_grid(cdiv_l(d.N, decltype(SPB)::value))), 0,
                part.data_ptr<float>(), w1.data_ptr<float>(),
                b1.data_ptr<float>(), w2t.data_ptr<float>(),
                b2.data_ptr<float>(), s.data_ptr<float>(),
                z.data_ptr<float>(), g.data_ptr<float>(), d, nchunks, flags);
    });
    launch256(se_apply_str<T16>, dim3(se_grid((long)d.N * bps)), 0,
              (const T16*)x.data_ptr(), g.data_ptr<float>(),
              (const T16*)res.data_ptr(), (T16*)y.data_ptr(),
              mask.data_ptr<unsigned char>(), d, bps, inv, flags);
  });
  if (!want_side) g = at::empty({0, d.C}, f32);
  return {y, s, z, g, mask};
}

// returns {dx, dres, dl[N,C], dz[N,Cr]}: dres is the masked dy when
// want_dres, else empty. mask: empty = no ReLU.
std::vector<at::Tensor> se_bwd(at::Tensor x, at::Tensor dy, at::Tensor mask,
                               at::Tensor z, at::Tensor g, at::Tensor w1,
                               at::Tensor w2t, bool want_dres, long path,
                               long chunk) {
  CHECK_GPU(x);
  CHECK_CONTIG(x);
  CHECK_GPU(dy);
  CHECK_CONTIG(dy);
  CHECK_16BIT(x);
  const SEDims d = se_dims(x, w1, w2t);
  TORCH_CHECK(dy.sizes() == x.sizes() && dy.scalar_type() == x.scalar_type(),
              "squeeze_excite: dy must match x");
  se_check_f32(z, (long)d.N * d.Cr, "z");
  se_check_f32(g, (long)d.N * d.C, "g");
  const bool has_mask = mask.numel() > 0;
  TORCH_CHECK(!has_mask || (mask.numel() == x.numel() / 8 && mask.is_cuda() &&
                            mask.scalar_type() == at::kByte),
              "squeeze_excite: mask must hold one bit per element");
  const int cfg = se_res_cfg(d, kBwdMaxNV);
  const int p = se_pick_path(path, cfg, "se_bwd");
  const int chunk_px = se_chunk_px(d, chunk, "se_bwd");
  const int nchunks = cdiv_i(d.HW, chunk_px);
  const int flags = (has_mask ? kMask : 0) | (want_dres ? kHasRes : 0);

  auto f32 = x.options().dtype(at::kFloat);
  auto dx = at::empty_like(x);
  auto dres = want_dres ? at::empty_like(x) : at::empty({0}, x.options());
  auto dl = at::empty({d.N, d.C}, f32), dz = at::empty({d.N, d.Cr}, f32);

  if (p == 1) {
    DISPATCH_16(x, T16, {
      pick<6401, 6402, 6404, 6408, 6416, 25601, 25602, 25604, 25608, 102402,
           102404, 102408>(
          cfg, [&](auto CFG) {
            constexpr int TS = decltype(CFG)::value / 100;
            constexpr int NV = decltype(CFG)::value % 100;
            constexpr int T = TS < 256 ? 256 : TS;
            hipLaunchKernelGGL(
                (se_bwd_res<T16, TS, NV>), dim3(se_grid(cdiv_l(d.N, T / TS))),
                dim3(T), 0, cur_stream(), (const T16*)x.data_ptr(),
                (const T16*)dy.data_ptr(),
                (const unsigned char*)mask.data_ptr<unsigned char>(),
                g.data_ptr<float>(), z.data_ptr<float>(),
                w1.data_ptr<float>(), w2t.data_ptr<float>(),
                (T16*)dx.data_ptr(), (T16*)dres.data_ptr(),
                dl.data_ptr<float>(), dz.data_ptr<float>(), d, flags);
          });
    });
    return {dx, dres, dl, dz};
  }
  auto part = at::empty({d.N, nchunks, d.C}, f32);
  auto ds = at::empty({d.N, d.C}, f32);
  int inv;
  const int bps = se_sweep_bps(d, inv);
  DISPATCH_16(x, T16, {
    launch256((se_sum_chunk<T16, true>), dim3(se_grid((long)d.N * nchunks)),
              0, (const T16*)x.data_ptr(), (const T16*)dy.data_ptr(),
              mask.data_ptr<unsigned char>(), part.data_ptr<float>(), d,
              nchunks, chunk_px, flags);
    pick<16, 4>(d.C <= 512 ? 16 : 4, [&](auto SPB) {
      launch256(se_gate_bwd_str<decltype(SPB)::value>,
                dim3(se_grid(cdiv_l(d.N, decltype(SPB)::value))), 0,
                part.data_ptr<float>(), g.data_ptr<float>(),
                z.data_ptr<float>(), w1.data_ptr<float>(),
                w2t.data_ptr<float>(), dl.data_ptr<float>(),
                dz.data_ptr<float>(), ds.data_ptr<float>(), d, nchunks);
    });
    launch256(se_bwd_dx_str<T16>, dim3(se_grid((long)d.N * bps)), 0,
              (const T16*)x.data_ptr(), (const T16*)dy.data_ptr(),
              mask.data_ptr<unsigned char>(), g.data_ptr<float>(),
              ds.data_ptr<float>(), (T16*)dx.data_ptr(),
              (T16*)dres.data_ptr(), d, bps, inv, flags);
  });
  return {dx, dres, dl, dz};
}

// returns {dw1[Cr,C], db1[Cr], dw2[C,Cr], db2[C]} from the fp32 side
// tensors: dw1 = dz^T s, db1 = sum_n dz, dw2 = dl^T z, db2 = sum_n dl.
std::vector<at::Tensor> se_wgrad(at::Tensor s, at::Tensor z, at::Tensor dl,
                                 at::Tensor dz) {
  TORCH_CHECK(s.dim() == 2 && z.dim() == 2 && s.size(0) == z.size(0) &&
                  s.size(0) >= 1,
              "se_wgrad: s must be [N,C] and z [N,Cr]");
  const long N = s.size(0), C = s.size(1), Cr = z.size(1);
  TORCH_CHECK(C >= 1 && C <= kMaxC && Cr >= 1 && Cr <= kMaxCr &&
                  N < (1L << 26),
              "se_wgrad: shape out of the domain");
  se_check_f32(s, N * C, "s");
  se_check_f32(z, N * Cr, "z");
  se_check_f32(dl, N * C, "dl");
  se_check_f32(dz, N * Cr, "dz");
  const SEDims d{(int)N, 1, (int)C, (int)Cr, (int)(C / 8)};
  constexpr int JPT = 8;
  const long gx = cdiv_l(C, 64), gy = cdiv_l(Cr, 4 * JPT);
  const long want = std::min<long>(std::max<long>(2048 / (gx * gy), 1), 64);
  const SplitPlan sp = split_plan(N, want);
  const long E = 2 * C * Cr + C + Cr;
  auto out = at::empty({E}, s.options());
  auto part = sp.n == 1 ? out : at::empty({sp.n, E}, s.options());
  launch256(se_wgrad_part<JPT>,
            dim3((unsigned)gx, (unsigned)gy, (unsigned)sp.n), 0,
            s.data_ptr<float>(), z.data_ptr<float>(), dl.data_ptr<float>(),
            dz.data_ptr<float>(), part.data_ptr<float>(), d, (int)sp.per, E);
  if (sp.n > 1) fold_rows(part, out, E, sp.n);
  const long o_b1 = Cr * C, o_w2 = o_b1 + Cr, o_b2 = o_w2 + C * Cr;
  return {out.narrow(0, 0, Cr * C).view({Cr, C}), out.narrow(0, o_b1, Cr),
          out.narrow(0, o_w2, C * Cr).view({C, Cr}), out.narrow(0, o_b2, C)};
}
