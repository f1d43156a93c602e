// GroupNorm over NHWC 16-bit activations, fp32 arithmetic (Wu & He 2018).
//
// Group g of sample n covers all H*W pixels of cpg = C/G channels, so a
// statistic never leaves one sample. The tensor is cut into (sample, slab)
// tiles, a slab being 64 channels (fewer when 64 does not divide C): a
// pixel row of a slab is one 128-byte line and a lane moves 16 B (8
// channels) of it.
//
// Resident path: a team of 64/256/1024 threads owns one tile and keeps it
// in REGISTERS (NV 16-byte vectors per lane, fully unrolled) from the one
// HBM read to the store of y or dx. Forward: mean, then sum (x-mean)^2 on
// the registers (a true two-pass variance), then the apply. Backward holds
// x and dy together, reduces A = sum d and Bx = sum d*xhat, and writes dx:
// one read of x and dy, one write. A 1024-thread team holds up to 128 KiB
// (8 vectors = 32 VGPRs per lane) in the forward; the backward is kept for
// tiles up to 8 KiB, where it measured faster than the streamed one. LDS
// holds only the cross-wave partial sums (a few KiB). Teams of 64 pack
// four small tiles into a 256-thread block.
//
// Streamed path (cpg > 64, tiles that do not fit): per (sample, slab,
// pixel-chunk) a chunk kernel computes (mean, M2) the same two-pass way on
// a register-resident chunk, a finalise kernel combines them in a fixed
// order (Chan et al.), and an elementwise kernel applies. Backward: chunk
// sums of A/Bx, a finalise, an elementwise dx.
//
// Every reduction has a fixed order: lane registers, wave shuffles, waves
// through LDS, rows through fold_rows. No float atomics; two runs give the
// same bits. Activation offsets are 64-bit, index decomposition is 32-bit.
#include "common.h"

// no packed-fp32 instructions in this file: per-element results must not
// depend on which v_pk_*_f32 form the scheduler picked
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

constexpr int kSlab = 64;  // channels per slab: one 128-byte line per pixel

struct GNDims {
  int HW, C, G;
  int cpg_log2;  // cpg is a power of two
  int S;         // slab channels: 64, or C's largest power-of-two divisor
  int lpr_log2;  // lanes per pixel row of a slab: S / 8 (1, 2, 4 or 8)
  int nslab;     // C / S
  int wseg;      // channels of a group inside one slab: min(cpg, S)
};

// Per-channel sums of NQ quantities over a team of TS threads. In: q[k][u],
// the lane's partial for slab channel (lane % lpr)*8 + u. The lanes of a
// wave that share a channel octet fold by shuffles, the team's waves meet
// in `red` and are added in wave order. Out: tot[k*64 + c], the team's
// total for slab channel c, times wgt[c] when given; the unweighted total
// also goes to out_row[k*out_stride + c] when given. All threads of the
// block must call this (it synchronises the block).
template <int TS, int NQ>
DEV_INLINE void team_channel_sums(float (&q)[NQ][8], float* red, float* tot,
                                  int lpr, int S, float* out_row,
                                  int out_stride, const float* wgt) {
  constexpr int WPT = TS / 64;
  const int t = threadIdx.x % TS, lane = t & 63;
  const int w = threadIdx.x >> 6;           // wave in block
  const int w0 = (threadIdx.x / TS) * WPT;  // the team's first wave
  for (int off = 32; off >= lpr; off >>= 1) {
#pragma unroll
    for (int k = 0; k < NQ; ++k)
#pragma unroll
      for (int u = 0; u < 8; ++u) q[k][u] += __shfl_xor(q[k][u], off, kWave);
  }
  __syncthreads();  // readers of the previous call's red/tot are done
  if (lane < lpr) {
#pragma unroll
    for (int k = 0; k < NQ; ++k)
#pragma unroll
      for (int u = 0; u < 8; ++u) red[(w * 2 + k) * 64 + lane * 8 + u] = q[k][u];
  }
  __syncthreads();
  for (int i = t; i < NQ * 64; i += TS) {
    const int k = i >> 6, c = i & 63;
    if (c < S) {
      float a = red[(w0 * 2 + k) * 64 + c];
      for (int wv = 1; wv < WPT; ++wv) a += red[((w0 + wv) * 2 + k) * 64 + c];
      if (out_row) out_row[(long)k * out_stride + c] = a;
      if (wgt) a *= wgt[c];
      tot[k * 64 + c] = a;
    }
  }
  __syncthreads();
}

// out[k][u] = sum of tot[k] over the wseg channels of the segment that
// holds the lane's channel lr*8 + u, added in channel order
template <int NQ>
DEV_INLINE void group_fold(const float* tot, int lr, int wseg,
                           float (&out)[NQ][8]) {
#pragma unroll
  for (int k = 0; k < NQ; ++k) {
    if (wseg >= 8) {  // the lane's 8 channels lie in one segment
      const int gb = (lr * 8) & ~(wseg - 1);
      float a = 0.f;
      for (int j = 0; j < wseg; ++j) a += tot[k * 64 + gb + j];
#pragma unroll
      for (int u = 0; u < 8; ++u) out[k][u] = a;
    } else {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int gb = (lr * 8 + u) & ~(wseg - 1);
        float a = 0.f;
        for (int j = 0; j < wseg; ++j) a += tot[k * 64 + gb + j];
        out[k][u] = a;
      }
    }
  }
}

// Two-pass (mean, M2 = sum (x-mean)^2) of every segment of a register-held
// set of vectors: xv[i] is valid where t + i*TS < V. Results per lane
// channel; `cnt` is the element count of a segment.
template <typename T16, int TS, int NV>
DEV_INLINE void two_pass_stats(const short8 (&xv)[NV], int t, int V, bool on,
                               float* red, float* tot, const GNDims& d,
                               float cnt, float (&mean)[1][8],
                               float (&m2)[1][8]) {
  const int lpr = 1 << d.lpr_log2, lr = t & (lpr - 1);
  float q[1][8] = {};
#pragma unroll
  for (int i = 0; i < NV; ++i)  // vectors past V hold zeros
#pragma unroll
    for (int u = 0; u < 8; ++u) q[0][u] += s16_to_f32<T16>(xv[i][u]);
  team_channel_sums<TS, 1>(q, red, tot, lpr, d.S, nullptr, 0, nullptr);
  group_fold<1>(tot, lr, d.wseg, mean);
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    mean[0][u] = mean[0][u] / cnt;
    q[0][u] = 0.f;
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (on && t + i * TS < V) {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const float c = s16_to_f32<T16>(xv[i][u]) - mean[0][u];
        q[0][u] += c * c;
      }
    }
  }
  team_channel_sums<TS, 1>(q, red, tot, lpr, d.S, nullptr, 0, nullptr);
  group_fold<1>(tot, lr, d.wseg, m2);
}

// ---- resident path ---------------------------------------------------------

#define GN_TEAM_SETUP                                                     \
  constexpr int T = TS < 256 ? 256 : TS;                                  \
  constexpr int TPB = T / TS; /* tiles per block */                       \
  __shared__ float red[(T / 64) * 2 * 64];                                \
  __shared__ float tots[TPB * 2 * 64];                                    \
  const int team = threadIdx.x / TS, t = threadIdx.x % TS;                \
  float* tot = tots + team * 2 * 64;                                      \
  const int tile_raw = blockIdx.x * TPB + team;                           \
  const bool on = tile_raw < ntiles; /* a team past the end idles */      \
  const int tile = on ? tile_raw : 0;                                     \
  const int n = tile / d.nslab, slab = tile - n * d.nslab;                \
  const int lpr = 1 << d.lpr_log2, lr = t & (lpr - 1);                    \
  const int V = d.HW << d.lpr_log2;      /* vectors in the tile */        \
  const int cb = slab * d.S + lr * 8;    /* the lane's first channel */   \
  const long base = (long)n * d.HW * d.C + cb

template <typename T16, int TS, int NV>
__global__ __launch_bounds__(TS < 256 ? 256 : TS) void gn_fwd_res(
    const T16* __restrict__ x, const float* __restrict__ gamma,
    const float* __restrict__ beta, const T16* __restrict__ res,
    T16* __restrict__ y, unsigned char* __restrict__ msk,
    float* __restrict__ mean_out, float* __restrict__ rstd_out, GNDims d,
    int ntiles, float eps, int act) {
  GN_TEAM_SETUP;
  short8 xv[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int v = t + i * TS;
    xv[i] = short8{};
    if (on && v < V)
      xv[i] = *reinterpret_cast<const short8*>(
          x + base + (long)(v >> d.lpr_log2) * d.C);
  }
  const float M = (float)(d.HW << d.cpg_log2);
  float mean[1][8], m2[1][8];
  two_pass_stats<T16, TS, NV>(xv, t, V, on, red, tot, d, M, mean, m2);
  float sc[8], bt[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const float rstd = 1.f / sqrtf(relu_f(m2[0][u] / M) + eps);
    const int c = cb + u;
    if (on && t < lpr && (c & ((1 << d.cpg_log2) - 1)) == 0) {
      mean_out[n * d.G + (c >> d.cpg_log2)] = mean[0][u];
      rstd_out[n * d.G + (c >> d.cpg_log2)] = rstd;
    }
    sc[u] = rstd * gamma[c];
    bt[u] = beta[c];
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int v = t + i * TS;
    if (on && v < V) {
      const long e = base + (long)(v >> d.lpr_log2) * d.C;
      short8 vr = {};
      if (res) vr = *reinterpret_cast<const short8*>(res + e);
      short8 o;
      unsigned mb = 0;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        float r = (s16_to_f32<T16>(xv[i][u]) - mean[0][u]) * sc[u] + bt[u];
        if (res) r += s16_to_f32<T16>(vr[u]);
        if (act == 1) r = relu_f(r);
        o[u] = f32_to_s16<T16>(r);
        if (s16_to_f32<T16>(o[u]) > 0.f) mb |= 1u << u;
      }
      *reinterpret_cast<short8*>(y + e) = o;
      if (msk) msk[e >> 3] = (unsigned char)mb;
    }
  }
}

template <typename T16, int TS, int NV>
__global__ __launch_bounds__(TS < 256 ? 256 : TS) void gn_bwd_res(
    const T16* __restrict__ x, const T16* __restrict__ dy,
    const unsigned char* __restrict__ msk, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ gamma,
    T16* __restrict__ dx, T16* __restrict__ dres,
    float* __restrict__ ab,  // [N][2][C]: A row, Bx row
    GNDims d, int ntiles) {
  GN_TEAM_SETUP;
  short8 xv[NV], dv[NV];  // dv holds the masked dy from here on
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int v = t + i * TS;
    xv[i] = short8{};
    dv[i] = short8{};
    if (on && v < V) {
      const long e = base + (long)(v >> d.lpr_log2) * d.C;
      xv[i] = *reinterpret_cast<const short8*>(x + e);
      dv[i] = *reinterpret_cast<const short8*>(dy + e);
      if (msk) {
        const unsigned mb = msk[e >> 3];
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (!((mb >> u) & 1)) dv[i][u] = 0;
      }
    }
  }
  float mu[8], rs[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int g = n * d.G + ((cb + u) >> d.cpg_log2);
    mu[u] = mean[g];
    rs[u] = rstd[g];
  }
  float q[2][8] = {};  // A, Bx
#pragma unroll
  for (int i = 0; i < NV; ++i)  // vectors past V hold zeros
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const float dd = s16_to_f32<T16>(dv[i][u]);
      q[0][u] += dd;
      q[1][u] += dd * ((s16_to_f32<T16>(xv[i][u]) - mu[u]) * rs[u]);
    }
  // keep the tile packed across the reduction: without this the compiler
  // carries fp32 copies of d and x - mean to the dx loop (twice the VGPRs)
#pragma unroll
  for (int i = 0; i < NV; ++i) asm volatile("" : "+v"(xv[i]), "+v"(dv[i]));
  team_channel_sums<TS, 2>(q, red, tot, lpr, d.S,
                           on ? ab + (long)n * 2 * d.C + slab * d.S : nullptr,
                           d.C, gamma + slab * d.S);
  group_fold<2>(tot, lr, d.wseg, q);  // s1, s2
  // dx = rstd*(gamma*d - (s1 + xhat*s2)/M) = k1*d - (c1 + (x-mean)*c2):
  // rs becomes k1 and q becomes (c1, c2), 32 live floats beside the tile
  const float M = (float)(d.HW << d.cpg_log2);
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const float k2 = rs[u] / M;
    q[0][u] *= k2;
    q[1][u] *= k2 * rs[u];
    rs[u] *= gamma[cb + u];
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int v = t + i * TS;
    if (on && v < V) {
      const long e = base + (long)(v >> d.lpr_log2) * d.C;
      short8 o;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const float dd = s16_to_f32<T16>(dv[i][u]);
        const float xc = s16_to_f32<T16>(xv[i][u]) - mu[u];
        o[u] = f32_to_s16<T16>(rs[u] * dd - (q[0][u] + xc * q[1][u]));
      }
      *reinterpret_cast<short8*>(dx + e) = o;
      if (dres) *reinterpret_cast<short8*>(dres + e) = dv[i];
    }
  }
}

// ---- streamed path ---------------------------------------------------------

constexpr int kChunkVec = 2048;  // vectors of a chunk: 8 per lane, 256 lanes

// one (sample, slab, chunk) per block: two-pass (mean, M2) of every segment
// (a group's channels inside this slab) on the register-held chunk
template <typename T16>
__global__ __launch_bounds__(256) void gn_stats_chunk(
    const T16* __restrict__ x, float* __restrict__ part,  // [N][nch][nseg][2]
    GNDims d, int nchunks, int chunk_px) {
  constexpr int TS = 256, NV = kChunkVec / 256;
  __shared__ float red[4 * 2 * 64];
  __shared__ float tot[2 * 64];
  const int t = threadIdx.x;
  const int tile = blockIdx.x / nchunks, ch = blockIdx.x - tile * nchunks;
  const int n = tile / d.nslab, slab = tile - n * d.nslab;
  const int lpr = 1 << d.lpr_log2, lr = t & (lpr - 1);
  const int p0 = ch * chunk_px, np = min(chunk_px, d.HW - p0);
  const int V = np << d.lpr_log2;
  const int cb = slab * d.S + lr * 8;
  const long base = ((long)n * d.HW + p0) * d.C + cb;
  short8 xv[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int v = t + i * TS;
    xv[i] = short8{};
    if (v < V)
      xv[i] = *reinterpret_cast<const short8*>(
          x + base + (long)(v >> d.lpr_log2) * d.C);
  }
  float mean[1][8], m2[1][8];
  two_pass_stats<T16, TS, NV>(xv, t, V, true, red, tot, d,
                              (float)(np * d.wseg), mean, m2);
  if (t < lpr) {
    const int nseg = d.C / d.wseg;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int c = cb + u;
      if (c % d.wseg == 0) {
        float* o = part + (((long)n * nchunks + ch) * nseg + c / d.wseg) * 2;
        o[0] = mean[0][u];
        o[1] = m2[0][u];
      }
    }
  }
}

// one thread per (sample, group): Chan's pairwise update over the group's
// chunks and segments, always in the same order
__global__ void gn_finalize_kernel(const float* __restrict__ part,
                                   float* __restrict__ mean_out,
                                   float* __restrict__ rstd_out, GNDims d,
                                   int N, int nchunks, int chunk_px,
                                   float eps) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * d.G) return;
  const int n = i / d.G, g = i - n * d.G;
  const int nseg = d.C / d.wseg, spg = (1 << d.cpg_log2) / d.wseg;
  float cnt = 0.f, mean = 0.f, m2 = 0.f;
  for (int ch = 0; ch < nchunks; ++ch) {
    const float nb =
        (float)(min(chunk_px, d.HW - ch * chunk_px) * d.wseg);
    const float* p = part + (((long)n * nchunks + ch) * nseg + g * spg) * 2;
    for (int s = 0; s < spg; ++s) {
      const float tn = cnt + nb, delta = p[2 * s] - mean;
      mean += delta * (nb / tn);
      m2 += p[2 * s + 1] + delta * delta * (cnt * nb / tn);
      cnt = tn;
    }
  }
  mean_out[i] = mean;
  rstd_out[i] = 1.f / sqrtf(relu_f(m2 / cnt) + eps);
}

// elementwise sweep of one sample per block row: blockIdx.x = n*bps + b.
// A thread's channel octet is the same for all its vectors when `inv`
// (its stride is a multiple of C/8): the parameters are loaded once.
#define GN_SWEEP_SETUP                                                    \
  const int n = blockIdx.x / bps, b = blockIdx.x - n * bps;               \
  const int cv = d.C >> 3, VS = d.HW * cv; /* vectors per sample */       \
  const long sbase = (long)n * d.HW * d.C;                                \
  const int stride = bps * 256;                                           \
  int v = b * 256 + threadIdx.x

template <typename T16>
__global__ __launch_bounds__(256) void gn_apply_str(
    const T16* __restrict__ x, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ gamma,
    const float* __restrict__ beta, const T16* __restrict__ res,
    T16* __restrict__ y, unsigned char* __restrict__ msk, GNDims d, int bps,
    int inv, int act) {
  GN_SWEEP_SETUP;
  float mu[8], sc[8], bt[8];
  auto params = [&](int c0) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int g = n * d.G + ((c0 + u) >> d.cpg_log2);
      mu[u] = mean[g];
      sc[u] = rstd[g] * gamma[c0 + u];
      bt[u] = beta[c0 + u];
    }
  };
  if (inv) params((v % cv) * 8);
  for (; v < VS; v += stride) {
    if (!inv) params((v % cv) * 8);
    const long e = sbase + (long)v * 8;
    const short8 vx = *reinterpret_cast<const short8*>(x + e);
    short8 vr = {};
    if (res) vr = *reinterpret_cast<const short8*>(res + e);
    short8 o;
    unsigned mb = 0;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      float r = (s16_to_f32<T16>(vx[u]) - mu[u]) * sc[u] + bt[u];
      if (res) r += s16_to_f32<T16>(vr[u]);
      if (act == 1) r = relu_f(r);
      o[u] = f32_to_s16<T16>(r);
      if (s16_to_f32<T16>(o[u]) > 0.f) mb |= 1u << u;
    }
    *reinterpret_cast<short8*>(y + e) = o;
    if (msk) msk[e >> 3] = (unsigned char)mb;
  }
}

// one (sample, slab, chunk) per block: per-channel A = sum d and
// Bx = sum d*xhat of the chunk into part[N][nch][2][C]
template <typename T16>
__global__ __launch_bounds__(256) void gn_bwd_reduce_str(
    const T16* __restrict__ x, const T16* __restrict__ dy,
    const unsigned char* __restrict__ msk, const float* __restrict__ mean,
    const float* __restrict__ rstd, float* __restrict__ part, GNDims d,
    int nchunks, int chunk_px) {
  __shared__ float red[4 * 2 * 64];
  __shared__ float tot[2 * 64];
  const int t = threadIdx.x;
  const int tile = blockIdx.x / nchunks, ch = blockIdx.x - tile * nchunks;
  const int n = tile / d.nslab, slab = tile - n * d.nslab;
  const int lpr = 1 << d.lpr_log2, lr = t & (lpr - 1);
  const int p0 = ch * chunk_px, np = min(chunk_px, d.HW - p0);
  const int V = np << d.lpr_log2;
  const int cb = slab * d.S + lr * 8;
  const long base = ((long)n * d.HW + p0) * d.C + cb;
  float mu[8], rs[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int g = n * d.G + ((cb + u) >> d.cpg_log2);
    mu[u] = mean[g];
    rs[u] = rstd[g];
  }
  float q[2][8] = {};
#pragma unroll 4
  for (int v = t; v < V; v += 256) {
    const long e = base + (long)(v >> d.lpr_log2) * d.C;
    const short8 vx = *reinterpret_cast<const short8*>(x + e);
    const short8 vd = *reinterpret_cast<const short8*>(dy + e);
    const unsigned mb = msk ? msk[e >> 3] : 0xffu;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const float dd = ((mb >> u) & 1) ? s16_to_f32<T16>(vd[u]) : 0.f;
      q[0][u] += dd;
      q[1][u] += dd * ((s16_to_f32<T16>(vx[u]) - mu[u]) * rs[u]);
    }
  }
  team_channel_sums<256, 2>(
      q, red, tot, lpr, d.S,
      part + ((long)n * nchunks + ch) * 2 * d.C + slab * d.S, d.C, nullptr);
}

// one thread per (sample, group): add the chunks of every channel of the
// group in order into ab[N][2][C], and s12[N*G][2] = (sum gamma*A,
// sum gamma*Bx) over the group
__global__ void gn_bwd_finalize_kernel(const float* __restrict__ part,
                                       const float* __restrict__ gamma,
                                       float* __restrict__ ab,
                                       float* __restrict__ s12, GNDims d,
                                       int N, int nchunks) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * d.G) return;
  const int n = i / d.G, g = i - n * d.G;
  const int cpg = 1 << d.cpg_log2;
  float s1 = 0.f, s2 = 0.f;
  for (int c = g * cpg; c < (g + 1) * cpg; ++c) {
    float a = 0.f, bx = 0.f;
    for (int ch = 0; ch < nchunks; ++ch) {
      const float* p = part + ((long)n * nchunks + ch) * 2 * d.C;
      a += p[c];
      bx += p[d.C + c];
    }
    ab[(long)n * 2 * d.C + c] = a;
    ab[(long)n * 2 * d.C + d.C + c] = bx;
    s1 += gamma[c] * a;
    s2 += gamma[c] * bx;
  }
  s12[2 * i] = s1;
  s12[2 * i + 1] = s2;
}

template <typename T16>
__global__ __launch_bounds__(256) void gn_bwd_dx_str(
    const T16* __restrict__ x, const T16* __restrict__ dy,
    const unsigned char* __restrict__ msk, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ gamma,
    const float* __restrict__ s12, T16* __restrict__ dx,
    T16* __restrict__ dres, GNDims d, int bps, int inv) {
  GN_SWEEP_SETUP;
  const float M = (float)d.HW * (float)(1 << d.cpg_log2);
  float mu[8], rs[8], k1[8], k2[8], s1[8], s2[8];
  auto params = [&](int c0) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int g = n * d.G + ((c0 + u) >> d.cpg_log2);
      mu[u] = mean[g];
      rs[u] = rstd[g];
      k1[u] = rs[u] * gamma[c0 + u];
      k2[u] = rs[u] / M;
      s1[u] = s12[2 * g];
      s2[u] = s12[2 * g + 1];
    }
  };
  if (inv) params((v % cv) * 8);
  for (; v < VS; v += stride) {
    if (!inv) params((v % cv) * 8);
    const long e = sbase + (long)v * 8;
    const short8 vx = *reinterpret_cast<const short8*>(x + e);
    short8 vd = *reinterpret_cast<const short8*>(dy + e);
    const unsigned mb = msk ? msk[e >> 3] : 0xffu;
    short8 o;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (!((mb >> u) & 1)) vd[u] = 0;
      const float dd = s16_to_f32<T16>(vd[u]);
      const float xh = (s16_to_f32<T16>(vx[u]) - mu[u]) * rs[u];
      o[u] = f32_to_s16<T16>(k1[u] * dd - k2[u] * (s1[u] + xh * s2[u]));
    }
    *reinterpret_cast<short8*>(dx + e) = o;
    if (dres) *reinterpret_cast<short8*>(dres + e) = vd;
  }
}

#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif

// ---- host ------------------------------------------------------------------

inline int ilog2(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}

GNDims gn_dims(const at::Tensor& x, long G) {
  TORCH_CHECK(x.dim() == 4, "group_norm: x must be NHWC [N,H,W,C]");
  const long C = x.size(3), HW = x.size(1) * x.size(2);
  TORCH_CHECK(C % 8 == 0, "group_norm: channels=", C,
              " must be a multiple of 8");
  TORCH_CHECK(G >= 1 && C % G == 0, "group_norm: num_groups=", G,
              " does not divide ", C, " channels");
  const long cpg = C / G;
  TORCH_CHECK((cpg & (cpg - 1)) == 0, "group_norm: channels per group=", cpg,
              " must be a power of two");
  TORCH_CHECK(HW >= 1 && HW * C < (1L << 31) && x.size(0) * G < (1L << 31),
              "group_norm: sample too large");
  GNDims d;
  d.HW = (int)HW;
  d.C = (int)C;
  d.G = (int)G;
  d.cpg_log2 = ilog2((int)cpg);
  // the largest power of two that divides C, 64 at most (cpg divides it
  // or is a multiple of 64): 64 for the usual widths, 32 for C = 96
  d.S = (int)std::min<long>(C & -C, kSlab);
  d.lpr_log2 = ilog2(d.S / 8);
  d.nslab = (int)(C / d.S);
  d.wseg = (int)std::min<long>(cpg, d.S);
  return d;
}

// Resident team shape for a tile of V vectors, as TS*100 + NV (0: the
// resident path does not serve it). A team of 64 serves up to 512 vectors
// (8 KiB), 256 up to 2048, 1024 up to 8192 (8 vectors per lane each).
int gn_res_cfg(const GNDims& d, long max_v) {
  if ((1 << d.cpg_log2) > kSlab) return 0;  // a group would leave its slab
  const long V = (long)d.HW << d.lpr_log2;
  if (V > max_v) return 0;
  const int ts = V <= 512 ? 64 : V <= 2048 ? 256 : 1024;
  int nv = ts == 64 ? 1 : 4;
  while ((long)nv * ts < V) nv *= 2;
  return ts * 100 + nv;
}

// The largest resident tile, in vectors. Forward: 8 per lane of a
// 1024-thread team (32x32x64, 128 KiB), all a lane's 128 VGPRs allow.
// Backward: teams of 64 only (8x8x64, x and dy 8 KiB each). Holding 8 + 8
// vectors takes 175 VGPRs, which spills in a 1024-thread team (the
// 32x32x64 backward), and the 256-thread team measured slower than the
// streamed backward at 16x16x128 (profiles/r14_groupnorm.md), so those
// variants were deleted.
constexpr long kFwdMaxV = 8192, kBwdMaxV = 512;

int gn_pick_path(long path, int cfg, const char* who) {
  TORCH_CHECK(path >= 0 && path <= 2, who, ": path must be 0, 1 or 2");
  TORCH_CHECK(path != 1 || cfg != 0, who,
              ": the resident path does not serve this shape");
  return path == 0 ? (cfg ? 1 : 2) : (int)path;
}

inline unsigned gn_tiles_grid(long tiles, int per_block) {
  const long blocks = cdiv_l(tiles, per_block);
  TORCH_CHECK(blocks < (1L << 31), "group_norm: too many tiles");
  return (unsigned)blocks;
}

// elementwise sweeps: blocks per sample (about four vectors per thread),
// and whether a thread's channel octet is stride-invariant
inline int gn_sweep_bps(const GNDims& d, int& inv) {
  const int cv = d.C / 8;
  inv = 256 % cv == 0;
  return (int)std::min<long>(cdiv_l((long)d.HW * cv, 1024), 1 << 16);
}

}  // namespace

// returns {y, mean[N,G], rstd[N,G], mask}: mask is bn_apply's 1-bit "y > 0"
// map when act == relu and want_mask, else empty. res: empty = none.
// path: 0 auto, 1 resident, 2 streamed; chunk: pixels per streamed chunk
// (0 auto).
std::vector<at::Tensor> gn_fwd(at::Tensor x, at::Tensor gamma,
                               at::Tensor beta, at::Tensor res, long G,
                               double eps, long act, bool want_mask,
                               long path, long chunk) {
  CHECK_GPU(x);
  CHECK_CONTIG(x);
  CHECK_16BIT(x);
  const GNDims d = gn_dims(x, G);
  const int N = x.size(0);
  TORCH_CHECK(gamma.numel() == d.C && beta.numel() == d.C &&
                  gamma.scalar_type() == at::kFloat &&
                  beta.scalar_type() == at::kFloat,
              "group_norm: gamma and beta must be fp32 [C]");
  const bool has_res = res.numel() > 0;
  TORCH_CHECK(!has_res || (res.sizes() == x.sizes() && res.is_contiguous() &&
                           res.scalar_type() == x.scalar_type()),
              "group_norm: residual must match x");
  const int cfg = gn_res_cfg(d, kFwdMaxV);
  const int p = gn_pick_path(path, cfg, "gn_fwd");
  const int max_chunk = kChunkVec >> d.lpr_log2;
  TORCH_CHECK(chunk >= 0 && chunk <= max_chunk, "gn_fwd: chunk=", chunk,
              " must be in [0, ", max_chunk, "]");
  const int chunk_px = chunk ? (int)chunk : max_chunk;
  const int nchunks = cdiv_i(d.HW, chunk_px);
  const long tiles = (long)N * d.nslab;

  auto f32 = x.options().dtype(at::kFloat);
  auto y = at::empty_like(x);
  auto mean = at::empty({N, d.G}, f32), rstd = at::empty({N, d.G}, f32);
  auto mask = (act == 1 && want_mask)
                  ? at::empty({x.numel() / 8}, x.options().dtype(at::kByte))
                  : at::empty({0}, x.options().dtype(at::kByte));
  unsigned char* mp = mask.numel() ? mask.data_ptr<unsigned char>() : nullptr;
  at::Tensor part;
  if (p == 2) part = at::empty({N, nchunks, d.C / d.wseg, 2}, f32);

  if (p == 1) {
    DISPATCH_16(x, T16, {
      pick<6401, 6402, 6404, 6408, 25604, 25608, 102404, 102408>(
          cfg, [&](auto CFG) {
            constexpr int TS = decltype(CFG)::value / 100;
            constexpr int NV = decltype(CFG)::value % 100;
            constexpr int T = TS < 256 ? 256 : TS;
            hipLaunchKernelGGL(
                (gn_fwd_res<T16, TS, NV>), dim3(gn_tiles_grid(tiles, T / TS)),
                dim3(T), 0, cur_stream(), (const T16*)x.data_ptr(),
                gamma.data_ptr<float>(), beta.data_ptr<float>(),
                has_res ? (const T16*)res.data_ptr() : nullptr,
                (T16*)y.data_ptr(), mp, mean.data_ptr<float>(),
                rstd.data_ptr<float>(), d, (int)tiles, (float)eps, (int)act);
          });
    });
    return {y, mean, rstd, mask};
  }
  int inv;
  const int bps = gn_sweep_bps(d, inv);
  DISPATCH_16(x, T16, {
    launch256(gn_stats_chunk<T16>, dim3(gn_tiles_grid(tiles * nchunks, 1)), 0,
              (const T16*)x.data_ptr(), part.data_ptr<float>(), d, nchunks,
              chunk_px);
    hipLaunchKernelGGL(gn_finalize_kernel, dim3(cdiv_i(N * d.G, 256)),
                       dim3(256), 0, cur_stream(), part.data_ptr<float>(),
                       mean.data_ptr<float>(), rstd.data_ptr<float>(), d, N,
                       nchunks, chunk_px, (float)eps);
    launch256(gn_apply_str<T16>, dim3(gn_tiles_grid((long)N * bps, 1)), 0,
              (const T16*)x.data_ptr(), mean.data_ptr<float>(),
              rstd.data_ptr<float>(), gamma.data_ptr<float>(),
              beta.data_ptr<float>(),
              has_res ? (const T16*)res.data_ptr() : nullptr,
              (T16*)y.data_ptr(), mp, d, bps, inv, (int)act);
  });
  return {y, mean, rstd, mask};
}

// returns {dx, dres, dgb}: dres is the masked dy when want_dres, else
// empty; dgb is [2, C] = (dbeta, dgamma). mask: empty = no ReLU.
std::vector<at::Tensor> gn_bwd(at::Tensor x, at::Tensor dy, at::Tensor mean,
                               at::Tensor rstd, at::Tensor gamma,
                               at::Tensor mask, long G, bool want_dres,
                               long path) {
  CHECK_GPU(x);
  CHECK_CONTIG(x);
  CHECK_CONTIG(dy);
  CHECK_16BIT(x);
  const GNDims d = gn_dims(x, G);
  const int N = x.size(0);
  TORCH_CHECK(dy.sizes() == x.sizes() && dy.scalar_type() == x.scalar_type(),
              "group_norm: dy must match x");
  TORCH_CHECK(mean.numel() == (long)N * d.G && rstd.numel() == (long)N * d.G &&
                  gamma.numel() == d.C && gamma.scalar_type() == at::kFloat,
              "group_norm: mean/rstd must be [N,G], gamma fp32 [C]");
  TORCH_CHECK(mask.numel() == 0 || mask.numel() == x.numel() / 8,
              "group_norm: mask must hold one bit per element");
  const int cfg = gn_res_cfg(d, kBwdMaxV);
  const int p = gn_pick_path(path, cfg, "gn_bwd");
  const int chunk_px = kChunkVec >> d.lpr_log2;
  const int nchunks = cdiv_i(d.HW, chunk_px);
  const long tiles = (long)N * d.nslab;

  auto f32 = x.options().dtype(at::kFloat);
  auto dx = at::empty_like(x);
  auto dres = want_dres ? at::empty_like(x) : at::empty({0}, x.options());
  auto ab = at::empty({N, 2, d.C}, f32);
  auto dgb = N == 1 ? ab.view({2, d.C}) : at::empty({2, d.C}, f32);
  const unsigned char* mp =
      mask.numel() ? mask.data_ptr<unsigned char>() : nullptr;
  at::Tensor part, s12;
  if (p == 2) {
    part = at::empty({N, nchunks, 2, d.C}, f32);
    s12 = at::empty({N * d.G, 2}, f32);
  }

  if (p == 1) {
    DISPATCH_16(x, T16, {
      pick<6401, 6402, 6404, 6408>(
          cfg, [&](auto CFG) {
            constexpr int TS = decltype(CFG)::value / 100;
            constexpr int NV = decltype(CFG)::value % 100;
            constexpr int T = TS < 256 ? 256 : TS;
            hipLaunchKernelGGL(
                (gn_bwd_res<T16, TS, NV>), dim3(gn_tiles_grid(tiles, T / TS)),
                dim3(T), 0, cur_stream(), (const T16*)x.data_ptr(),
                (const T16*)dy.data_ptr(), mp, mean.data_ptr<float>(),
                rstd.data_ptr<float>(), gamma.data_ptr<float>(),
                (T16*)dx.data_ptr(),
                want_dres ? (T16*)dres.data_ptr() : nullptr,
                ab.data_ptr<float>(), d, (int)tiles);
          });
    });
  } else {
    int inv;
    const int bps = gn_sweep_bps(d, inv);
    DISPATCH_16(x, T16, {
      launch256(gn_bwd_reduce_str<T16>,
                dim3(gn_tiles_grid(tiles * nchunks, 1)), 0,
                (const T16*)x.data_ptr(), (const T16*)dy.data_ptr(), mp,
                mean.data_ptr<float>(), rstd.data_ptr<float>(),
                part.data_ptr<float>(), d, nchunks, chunk_px);
      hipLaunchKernelGGL(gn_bwd_finalize_kernel, dim3(cdiv_i(N * d.G, 256)),
                         dim3(256), 0, cur_stream(), part.data_ptr<float>(),
                         gamma.data_ptr<float>(), ab.data_ptr<float>(),
                         s12.data_ptr<float>(), d, N, nchunks);
      launch256(gn_bwd_dx_str<T16>, dim3(gn_tiles_grid((long)N * bps, 1)), 0,
                (const T16*)x.data_ptr(), (const T16*)dy.data_ptr(), mp,
                mean.data_ptr<float>(), rstd.data_ptr<float>(),
                gamma.data_ptr<float>(), s12.data_ptr<float>(),
                (T16*)dx.data_ptr(),
                want_dres ? (T16*)dres.data_ptr() : nullptr, d, bps, inv);
    });
  }
  // dbeta_c = sum_n A, dgamma_c = sum_n Bx: the [N][2C] rows in row order
  if (N > 1) fold_rows(ab, dgb, 2L * d.C, N);
  return {dx, dres, dgb};
}
