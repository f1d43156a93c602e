// LayerNorm over the last dimension of a contiguous [M, D] 16-bit tensor,
// fp32 arithmetic, with the pre-norm residual add fused in:
//
//     s = x + r                    (rounded once to the 16-bit type, stored)
//     y = (s - mean) * rstd * gamma + beta         (statistics of the stored s)
//
// so y == LN(s as stored) and the backward recomputes xhat from s alone.
//
// A row never leaves one wave. A group of L lanes (a power of two, 4..64)
// owns a row; lane l holds NV 16-byte vectors (8 elements each), vector j of
// lane l being row vector j*L + l, so each of the NV loads of a group is one
// contiguous run of L*16 bytes. A wave serves 64/L rows at once and a
// 256-thread block 4*64/L. Row statistics are folded with xor-shuffles over
// the L lanes: no LDS and no block barrier in the row reduction. When
// D/8 < L*NV the trailing vectors are masked: no load, zero contribution,
// no store.
//
// Which (L, NV) serves a D (ln_plan below): with V = D/8 vectors, for every
// NV in 1..8 take L = the smallest power of two >= max(4, ceil(V/NV)), at
// most 64, and keep the pair with the fewest masked vectors L*NV - V; among
// equals the smallest NV (more rows in flight per register). D = 256 is
// 32 x 1, 384 is 16 x 3, 768 is 32 x 3, 4064 and 4096 are 64 x 8. L is a
// kernel argument and NV a template argument (unrolled). The bindings take
// an NV override so that two plausible shapes can be measured
// (benchmarks/ln_bench.py); ops.layer_norm always passes 0 = the rule.
//
// Forward: one read of x (and r), mean, then sum (s-mean)^2 on the
// registers (a true two-pass variance), one write of y (and s).
//
// Backward, one kernel: s, dy and ds of a row are held in registers
// together. dxhat = dy*gamma,
//     d = rstd * (dxhat - mean_row(dxhat) - xhat * mean_row(dxhat*xhat)) + ds
// is written once; it is the gradient of both x and r. A block walks a
// contiguous range of rows and keeps its per-column sums of dy*xhat and dy
// in registers. At the end the 64/L row slots of a wave fold by shuffles
// (offsets L, 2L, .. 32), waves 1..3 hand their sums to wave 0 through LDS,
// which adds them in wave order and writes one fp32 row of partials
// [2][D]; fold_rows (common.h) then adds the partial rows in a fixed
// order. No atomics: two runs give the same bits. The number of partial
// rows is at most 4 per CU, whatever M is.
//
// Activation offsets are 64-bit. Everything is launched on the current
// stream and allocates only torch outputs, so the op can be captured.
#include "common.h"

// no packed-fp32 instructions in this file: per-element results must not
// depend on which v_pk_*_f32 form the scheduler picked
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

constexpr int kLNWaves = 4;    // waves of a block
constexpr int kLNMaxNV = 8;    // vectors per lane
constexpr int kLNPartsPerCU = 4;

// sum over the L lanes that own one row; every lane of the wave calls it
DEV_INLINE float ln_row_sum(float v, int L) {
  for (int off = L >> 1; off; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

DEV_INLINE void ln_load8(const float* __restrict__ p, float (&o)[8]) {
  const float4v a = *reinterpret_cast<const float4v*>(p);
  const float4v b = *reinterpret_cast<const float4v*>(p + 4);
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    o[u] = a[u];
    o[4 + u] = b[u];
  }
}

// where a lane stands: its row slot in the wave and its place in the row
struct LNLane {
  int L, l, wave, slot, rpw;
  DEV_INLINE explicit LNLane(int llog2) {
    const int lane = threadIdx.x & 63;
    L = 1 << llog2;
    l = lane & (L - 1);
    slot = lane >> llog2;
    rpw = 64 >> llog2;
    wave = threadIdx.x >> 6;
  }
};

template <typename T16, int NV, bool ADD>
__global__ __launch_bounds__(kLNWaves * 64) void ln_fwd_kernel(
    const T16* __restrict__ x, const T16* __restrict__ r,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    T16* __restrict__ s_out, T16* __restrict__ y, float* __restrict__ mean_out,
    float* __restrict__ rstd_out, int M, int D, int llog2, float eps) {
  const LNLane p(llog2);
  const int V = D >> 3;
  const long row = ((long)blockIdx.x * kLNWaves + p.wave) * p.rpw + p.slot;
  const bool on = row < M;
  const long base = row * D;
  short8 sv[NV];
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int v = j * p.L + p.l;
    sv[j] = short8{};
    if (on && v < V) {
      const long e = base + (long)v * 8;
      sv[j] = *reinterpret_cast<const short8*>(x + e);
      if constexpr (ADD) {
        const short8 rv = *reinterpret_cast<const short8*>(r + e);
#pragma unroll
        for (int u = 0; u < 8; ++u)
          sv[j][u] = f32_to_s16<T16>(s16_to_f32<T16>(sv[j][u]) +
                                     s16_to_f32<T16>(rv[u]));
        *reinterpret_cast<short8*>(s_out + e) = sv[j];
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) sum += s16_to_f32<T16>(sv[j][u]);  // 0 if off
  }
  const float mean = ln_row_sum(sum, p.L) / (float)D;
  float m2 = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    if (on && j * p.L + p.l < V) {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const float c = s16_to_f32<T16>(sv[j][u]) - mean;
        m2 += c * c;
      }
    }
  }
  const float rstd = 1.f / sqrtf(ln_row_sum(m2, p.L) / (float)D + eps);
  if (on && p.l == 0) {
    mean_out[row] = mean;
    rstd_out[row] = rstd;
  }
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int v = j * p.L + p.l;
    if (on && v < V) {
      float gm[8], bt[8];
      ln_load8(gamma + v * 8, gm);
      ln_load8(beta + v * 8, bt);
      short8 o;
#pragma unroll
      for (int u = 0; u < 8; ++u)
        o[u] = f32_to_s16<T16>(
            (s16_to_f32<T16>(sv[j][u]) - mean) * (rstd * gm[u]) + bt[u]);
      *reinterpret_cast<short8*>(y + base + (long)v * 8) = o;
    }
  }
}

// One quantity's per-column sums of a block -> row `out` of the partials.
// In: q[j][u], already folded over the wave's row slots (lanes < L hold it).
// All threads of the block call this.
template <int NV>
DEV_INLINE void ln_block_columns(const float (&q)[NV][8], float* lds,
                                 const LNLane& p, int V,
                                 float* __restrict__ out) {
  __syncthreads();  // wave 0 has read the previous quantity
  if (p.wave > 0 && p.slot == 0) {
#pragma unroll
    for (int j = 0; j < NV; ++j)
#pragma unroll
      for (int u = 0; u < 8; ++u)
        lds[(((p.wave - 1) * NV + j) * p.L + p.l) * 8 + u] = q[j][u];
  }
  __syncthreads();
  if (p.wave == 0 && p.slot == 0) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int v = j * p.L + p.l;
      if (v < V) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          float a = q[j][u];
          for (int w = 0; w < kLNWaves - 1; ++w)
            a += lds[((w * NV + j) * p.L + p.l) * 8 + u];
          out[v * 8 + u] = a;
        }
      }
    }
  }
}

template <typename T16, int NV, bool DS>
__global__ __launch_bounds__(kLNWaves * 64) void ln_bwd_kernel(
    const T16* __restrict__ s, const T16* __restrict__ dy,
    const T16* __restrict__ ds, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ gamma,
    T16* __restrict__ d, float* __restrict__ part,  // [blocks][2][D]
    int M, int D, int llog2, int rows_per_block) {
  extern __shared__ float lds[];  // [3 waves][NV][L][8]
  const LNLane p(llog2);
  const int V = D >> 3;
  const long r0 = (long)blockIdx.x * rows_per_block;
  const long rend = min(r0 + rows_per_block, (long)M);
  const float fD = (float)D;
  float ag[NV][8] = {}, ab[NV][8] = {};  // sums of dy*xhat and of dy
  for (long rb = r0; rb < rend; rb += kLNWaves * p.rpw) {
    const long row = rb + p.wave * p.rpw + p.slot;
    const bool on = row < rend;
    const long base = row * D;
    const float mu = on ? mean[row] : 0.f, rs = on ? rstd[row] : 0.f;
    short8 sv[NV], dv[NV], tv[DS ? NV : 1];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int v = j * p.L + p.l;
      sv[j] = short8{};
      dv[j] = short8{};
      if constexpr (DS) tv[j] = short8{};
      if (on && v < V) {
        const long e = base + (long)v * 8;
        sv[j] = *reinterpret_cast<const short8*>(s + e);
        dv[j] = *reinterpret_cast<const short8*>(dy + e);
        if constexpr (DS) tv[j] = *reinterpret_cast<const short8*>(ds + e);
      }
    }
    float c1 = 0.f, c2 = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int v = j * p.L + p.l;
      float gm[8] = {};
      if (v < V) ln_load8(gamma + v * 8, gm);
#pragma unroll
      for (int u = 0; u < 8; ++u) {  // a masked vector has dy = 0
        const float dd = s16_to_f32<T16>(dv[j][u]);
        const float xh = (s16_to_f32<T16>(sv[j][u]) - mu) * rs;
        const float g = dd * gm[u];
        c1 += g;
        c2 += g * xh;
        ag[j][u] += dd * xh;
        ab[j][u] += dd;
      }
    }
    // keep the row packed across the reduction (as gn_bwd_res does)
#pragma unroll
    for (int j = 0; j < NV; ++j) asm volatile("" : "+v"(sv[j]), "+v"(dv[j]));
    c1 = ln_row_sum(c1, p.L) / fD;
    c2 = ln_row_sum(c2, p.L) / fD;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int v = j * p.L + p.l;
      if (on && v < V) {
        float gm[8];
        ln_load8(gamma + v * 8, gm);
        short8 o;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const float xh = (s16_to_f32<T16>(sv[j][u]) - mu) * rs;
          float r = rs * (s16_to_f32<T16>(dv[j][u]) * gm[u] - c1 - xh * c2);
          if constexpr (DS) r += s16_to_f32<T16>(tv[j][u]);
          o[u] = f32_to_s16<T16>(r);
        }
        *reinterpret_cast<short8*>(d + base + (long)v * 8) = o;
      }
    }
  }
  // the wave's row slots own the same columns: fold them, lowest offset first
  for (int off = p.L; off < 64; off <<= 1) {
#pragma unroll
    for (int j = 0; j < NV; ++j)
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        ag[j][u] += __shfl_xor(ag[j][u], off, kWave);
        ab[j][u] += __shfl_xor(ab[j][u], off, kWave);
      }
  }
  float* out = part + (long)blockIdx.x * 2 * D;
  ln_block_columns<NV>(ag, lds, p, V, out);
  ln_block_columns<NV>(ab, lds, p, V, out + D);
}

#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif

// ---- host ------------------------------------------------------------------

struct LNPlan {
  int llog2, nv;
};

// the (L, NV) rule of the file header; nv_force != 0 fixes NV
LNPlan ln_plan(long D, long nv_force, const char* who) {
  TORCH_CHECK(D % 32 == 0 && D >= 32 && D <= 4096, who, ": D=", D,
              " must be a multiple of 32 in [32, 4096]");
  TORCH_CHECK(nv_force >= 0 && nv_force <= kLNMaxNV, who, ": nv=", nv_force,
              " must be in [0, ", kLNMaxNV, "]");
  const int V = (int)(D / 8);
  LNPlan best{0, 0};
  int best_pad = 1 << 30;
  for (int nv = 1; nv <= kLNMaxNV; ++nv) {
    if (nv_force && nv != nv_force) continue;
    int llog2 = 2;
    while ((1 << llog2) < cdiv_i(V, nv)) ++llog2;
    if (llog2 > 6) continue;
    const int pad = (nv << llog2) - V;
    if (pad < best_pad) {
      best_pad = pad;
      best = {llog2, nv};
    }
  }
  TORCH_CHECK(best.nv, who, ": nv=", nv_force, " cannot hold D=", D);
  return best;
}

unsigned ln_grid(long blocks) {
  TORCH_CHECK(blocks < (1L << 31), "layer_norm: too many rows");
  return (unsigned)blocks;
}

}  // namespace

// x [M, D]; r: empty = no fused add. Returns {y, s, mean[M], rstd[M]}; s is
// empty without r. nv: 0 = the rule, else the vectors per lane.
std::vector<at::Tensor> ln_fwd(at::Tensor x, at::Tensor r, at::Tensor gamma,
                               at::Tensor beta, double eps, long nv) {
  CHECK_GPU(x);
  CHECK_CONTIG(x);
  CHECK_16BIT(x);
  TORCH_CHECK(x.dim() == 2 && x.size(0) >= 1, "layer_norm: x must be [M, D]");
  const long M = x.size(0), D = x.size(1);
  TORCH_CHECK(M < (1L << 31), "layer_norm: too many rows");
  const LNPlan pl = ln_plan(D, nv, "ln_fwd");
  TORCH_CHECK(gamma.numel() == D && beta.numel() == D && gamma.is_cuda() &&
                  beta.is_cuda() && gamma.is_contiguous() &&
                  beta.is_contiguous() && gamma.scalar_type() == at::kFloat &&
                  beta.scalar_type() == at::kFloat,
              "layer_norm: gamma and beta must be fp32 [D]");
  const bool add = r.numel() > 0;
  TORCH_CHECK(!add || (r.sizes() == x.sizes() && r.is_contiguous() &&
                       r.is_cuda() && r.scalar_type() == x.scalar_type()),
              "layer_norm: residual must match x");
  auto f32 = x.options().dtype(at::kFloat);
  auto y = at::empty_like(x);
  auto s = add ? at::empty_like(x) : at::empty({0}, x.options());
  auto mean = at::empty({M}, f32), rstd = at::empty({M}, f32);
  const int rpb = kLNWaves * (64 >> pl.llog2);
  const unsigned grid = ln_grid(cdiv_l(M, rpb));
  DISPATCH_16(x, T16, {
    pick<1, 2, 3, 4, 5, 6, 7, 8>(pl.nv, [&](auto NV) {
      pick<false, true>(add, [&](auto ADD) {
        launch256(ln_fwd_kernel<T16, decltype(NV)::value, decltype(ADD)::value>,
                  dim3(grid), 0, (const T16*)x.data_ptr(),
                  add ? (const T16*)r.data_ptr() : nullptr,
                  gamma.data_ptr<float>(), beta.data_ptr<float>(),
                  add ? (T16*)s.data_ptr() : nullptr, (T16*)y.data_ptr(),
                  mean.data_ptr<float>(), rstd.data_ptr<float>(), (int)M,
                  (int)D, pl.llog2, (float)eps);
      });
    });
  });
  return {y, s, mean, rstd};
}

// s [M, D] as stored by the forward (x itself without a residual); ds: the
// gradient arriving on s, empty = none. Returns {d, dgb}: d is the gradient
// of x and of r, dgb is [2, D] = (dgamma, dbeta).
std::vector<at::Tensor> ln_bwd(at::Tensor s, at::Tensor dy, at::Tensor ds,
                               at::Tensor mean, at::Tensor rstd,
                               at::Tensor gamma, long nv) {
  CHECK_GPU(s);
  CHECK_CONTIG(s);
  CHECK_16BIT(s);
  TORCH_CHECK(s.dim() == 2 && s.size(0) >= 1, "layer_norm: s must be [M, D]");
  const long M = s.size(0), D = s.size(1);
  TORCH_CHECK(M < (1L << 31), "layer_norm: too many rows");
  const LNPlan pl = ln_plan(D, nv, "ln_bwd");
  const bool has_ds = ds.numel() > 0;
  for (const at::Tensor* t : {&dy, &ds}) {
    if (t == &ds && !has_ds) continue;
    TORCH_CHECK(t->is_cuda() && t->is_contiguous() &&
                    t->sizes() == s.sizes() &&
                    t->scalar_type() == s.scalar_type(),
                "layer_norm: dy and ds must match s");
  }
  TORCH_CHECK(mean.numel() == M && rstd.numel() == M && mean.is_cuda() &&
                  rstd.is_cuda() && mean.scalar_type() == at::kFloat &&
                  rstd.scalar_type() == at::kFloat && gamma.numel() == D &&
                  gamma.is_cuda() && gamma.is_contiguous() &&
                  gamma.scalar_type() == at::kFloat,
              "layer_norm: mean/rstd must be fp32 [M], gamma fp32 [D]");
  const int L = 1 << pl.llog2, rpb = kLNWaves * (64 >> pl.llog2);
  const long cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  const SplitPlan sp = split_plan(M, kLNPartsPerCU * cus, rpb);

  auto f32 = s.options().dtype(at::kFloat);
  auto d = at::empty_like(s);
  auto part = at::empty({sp.n, 2, D}, f32);
  auto dgb = sp.n == 1 ? part.view({2, D}) : at::empty({2, D}, f32);
  const size_t lds = sizeof(float) * (kLNWaves - 1) * pl.nv * L * 8;
  DISPATCH_16(s, T16, {
    pick<1, 2, 3, 4, 5, 6, 7, 8>(pl.nv, [&](auto NV) {
      pick<false, true>(has_ds, [&](auto DS) {
        launch256(ln_bwd_kernel<T16, decltype(NV)::value, decltype(DS)::value>,
                  dim3(ln_grid(sp.n)), lds, (const T16*)s.data_ptr(),
                  (const T16*)dy.data_ptr(),
                  has_ds ? (const T16*)ds.data_ptr() : nullptr,
                  mean.data_ptr<float>(), rstd.data_ptr<float>(),
                  gamma.data_ptr<float>(), (T16*)d.data_ptr(),
                  part.data_ptr<float>(), (int)M, (int)D, pl.llog2,
                  (int)sp.per);
      });
    });
  });
  if (sp.n > 1) fold_rows(part, dgb, 2 * D, sp.n);
  return {d, dgb};
}
