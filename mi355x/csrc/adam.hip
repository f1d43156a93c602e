// AdamW and LAMB (You et al. 2020) over the flat fp32 buffers, on the tile
// plan of lars.hip (tile_plan.h): tiles of at most kTile elements that never
// cross a tensor boundary, each a scalar head up to 16-byte alignment, a
// 16 B/lane body and a scalar tail.
//
// With g = g_raw * eff (eff from the guard state, guard.h) and t = the
// applied steps so far + 1, read from the step clock:
//
//   m = b1*m + (1-b1)*g            v = b2*v + (1-b2)*g*g
//   u = (m / (1-b1^t)) / (sqrt(v / (1-b2^t)) + eps) + wd_s*w
//   AdamW   w -= lr * u
//   LAMB    w -= lr * trust_s * u, trust_s = ||w_s|| / ||u_s||
//           (1 for an excluded tensor, or if either norm is 0)
//
// wd_s = 0 for an excluded tensor. Every thread forms 1/(1-b1^t) and
// 1/sqrt(1-b2^t) once, in double, from the clock's step: no step counter
// lives on the host, and a step skipped for an inf/nan gradient (grad_stats
// ran before and left the count in the guard state) writes nothing and does
// not move t, because clock_advance does not advance either.
//
// One kernel template walks the plan for all three passes:
//
//   kFused    AdamW: reads g w m v (e), writes m v w (e)        4 + 3 floats
//   kMoments  LAMB 1: reads g w m v, writes m v; u stays in registers and
//             w^2, u^2 go per tile into the slab (lanes, then
//             block_sum256 of reduce.h: one fixed order)        4 + 2
//   kApply    LAMB 2: reads w m v (e), recomputes u from the stored moments
//             with the same operations, writes w (e)            3 + 1
//
// Between the LAMB passes one block adds each tensor's tiles in tile order in
// double (combine_tiles, tile_plan.h, shared with lars_finalise_kernel) and
// writes {||w_s||, ||u_s||, trust_s} into the plan's stats. No
// float atomics, no last-block ticket: two runs, and two ranks that hold the
// same gradient, give the same bits for any grid.
#include "common.h"
#include "guard.h"
#include "tile_plan.h"

#include <climits>
#include <cmath>
#include <cstdint>

// no packed-fp32 instructions in this file (see gn.hip)
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

enum Pass { kFused = 0, kMoments = 1, kApply = 2 };

struct AdamCoef {
  float b1, omb1, b2, omb2;  // the betas and 1 - beta, rounded on the host
  float rbc1, rsbc2;         // 1/(1-b1^t), 1/sqrt(1-b2^t)
  float eps;
};

// b^t by squaring, in double: the CPU twin does the same multiplications
DEV_INLINE double ipow(double b, int t) {
  double r = 1.0;
  for (; t > 0; t >>= 1) {
    if (t & 1) r *= b;
    b *= b;
  }
  return r;
}

DEV_INLINE AdamCoef adam_coef(const float* __restrict__ clock, double b1,
                              double b2, float eps) {
  const int done = reinterpret_cast<const int*>(clock)[kClkStep];
  const int t = done < INT_MAX ? max(done, 0) + 1 : INT_MAX;
  AdamCoef c;
  c.b1 = (float)b1;
  c.omb1 = (float)(1.0 - b1);
  c.b2 = (float)b2;
  c.omb2 = (float)(1.0 - b2);
  c.rbc1 = (float)(1.0 / (1.0 - ipow(b1, t)));
  c.rsbc2 = (float)(1.0 / sqrt(1.0 - ipow(b2, t)));
  c.eps = eps;
  return c;
}

// every rounding spelled out, so kApply recomputes kMoments' u to the bit
DEV_INLINE void adam_moments(float& m, float& v, float g_raw, float eff,
                             const AdamCoef& c) {
#pragma clang fp contract(off)
  const float g = g_raw * eff;
  m = fmaf(c.b1, m, c.omb1 * g);
  v = fmaf(c.b2, v, (c.omb2 * g) * g);
}

DEV_INLINE float adam_u(float w, float m, float v, float wd,
                        const AdamCoef& c) {
#pragma clang fp contract(off)
  const float den = fmaf(sqrtf(v), c.rsbc2, c.eps);
  return fmaf(wd, w, (m * c.rbc1) / den);
}

// what is the same for every element of a tile
struct TileCoef {
  float eff, wd, step, omd;  // step = lr * trust_s
};

template <int kPass, bool kEma>
DEV_INLINE void adam_elem(float& w, float g, float& m, float& v, float& e,
                          float& sw, float& su, const AdamCoef& c,
                          const TileCoef& q) {
#pragma clang fp contract(off)
  if constexpr (kPass != kApply) adam_moments(m, v, g, q.eff, c);
  const float u = adam_u(w, m, v, q.wd, c);
  if constexpr (kPass == kMoments) {
    sw = fmaf(w, w, sw);
    su = fmaf(u, u, su);
  } else {
    w = fmaf(-q.step, u, w);
    if constexpr (kEma) ema_elem(e, w, q.omd);
  }
}

// g is read unless kPass == kApply; m and v are written unless kApply; w
// (and e with kEma) unless kMoments, which writes slab_w[t], slab_u[t]
// instead. kEma is only built for the passes that write w.
template <int kPass, bool kEma>
__global__ __launch_bounds__(256) void adam_tiles_kernel(
    float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m,
    float* __restrict__ v, long n, const int4v* __restrict__ table, int T,
    const int4v* __restrict__ tens, int S, const float* __restrict__ st,
    const float* __restrict__ stats, const float* __restrict__ clock,
    const float* __restrict__ lr_dev, float lr_host, double b1, double b2,
    float eps, float wd_host, float gscale_host, float max_norm,
    float* __restrict__ e, float* __restrict__ slab_w,
    float* __restrict__ slab_u) {
  static_assert(!(kEma && kPass == kMoments), "the moments pass writes no w");
  if (reinterpret_cast<const int*>(st)[kNonFinite] != 0) return;  // skipped: no write
  const AdamCoef c = adam_coef(clock, b1, b2, eps);
  const float lr = lr_dev ? *lr_dev : lr_host;
  TileCoef qc;
  qc.eff = guard_coef(st, gscale_host, max_norm).eff;
  qc.omd = 0.f;
  if constexpr (kEma) qc.omd = clock[kClkEmaOmd];
  const int tid = threadIdx.x;
  for (int t = blockIdx.x; t < T; t += gridDim.x) {
    const Tile q = load_tile(table, t, n, S);
    float aw[4] = {0.f, 0.f, 0.f, 0.f}, au[4] = {0.f, 0.f, 0.f, 0.f};
    if (q.ok) {
      qc.wd = tens[q.tensor][2] ? 0.f : wd_host;
      qc.step = lr;
      if constexpr (kPass == kApply) qc.step = lr * stats[3 * q.tensor + 2];
      float* wt = w + q.start;
      const float* gt = g + q.start;
      float* mt = m + q.start;
      float* vt = v + q.start;
      float* et = nullptr;
      if constexpr (kEma) et = e + q.start;

      auto scalar = [&](int i) {
        float a = wt[i], b = mt[i], d = vt[i], x = 0.f, y = 0.f;
        if constexpr (kPass != kApply) x = gt[i];
        if constexpr (kEma) y = et[i];
        adam_elem<kPass, kEma>(a, x, b, d, y, aw[0], au[0], c, qc);
        if constexpr (kPass != kApply) {
          mt[i] = b;
          vt[i] = d;
        }
        if constexpr (kPass != kMoments) wt[i] = a;
        if constexpr (kEma) et[i] = y;
      };

      if (tid < q.head) scalar(tid);
      float4v* wv = reinterpret_cast<float4v*>(wt + q.head);
      const float4v* gv = reinterpret_cast<const float4v*>(gt + q.head);
      float4v* mv = reinterpret_cast<float4v*>(mt + q.head);
      float4v* vv = reinterpret_cast<float4v*>(vt + q.head);
      float4v* ev = nullptr;
      if constexpr (kEma) ev = reinterpret_cast<float4v*>(et + q.head);
      // every load of the tile is issued before the first use
      float4v xw[kVecs], xg[kVecs], xm[kVecs], xv[kVecs], xe[kVecs];
#pragma unroll
      for (int k = 0; k < kVecs; ++k) {
        const int i = tid + k * 256;
        if (i < q.nvec) {
          if constexpr (kPass != kApply) xg[k] = gv[i];
          xw[k] = wv[i];
          xm[k] = mv[i];
          xv[k] = vv[i];
          if constexpr (kEma) xe[k] = ev[i];
        }
      }
#pragma unroll
      for (int k = 0; k < kVecs; ++k) {
        const int i = tid + k * 256;
        if (i < q.nvec) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float a = xw[k][j], b = xm[k][j], d = xv[k][j], x = 0.f, y = 0.f;
            if constexpr (kPass != kApply) x = xg[k][j];
            if constexpr (kEma) y = xe[k][j];
            adam_elem<kPass, kEma>(a, x, b, d, y, aw[j], au[j], c, qc);
            xw[k][j] = a;
            xm[k][j] = b;
            xv[k][j] = d;
            if constexpr (kEma) xe[k][j] = y;
          }
          if constexpr (kPass != kApply) {
            mv[i] = xm[k];
            vv[i] = xv[k];
          }
          if constexpr (kPass != kMoments) wv[i] = xw[k];
          if constexpr (kEma) ev[i] = xe[k];
        }
      }
      if (tid < q.tail) scalar(q.head + 4 * q.nvec + tid);
    }
    if constexpr (kPass == kMoments) {
      // a tile that cannot be read adds 0 to its tensor's sums
      float sw = sum4(aw[0], aw[1], aw[2], aw[3]);
      float su = sum4(au[0], au[1], au[2], au[3]);
      block_sum256(sw, su);
      if (tid == 0) {
        slab_w[t] = sw;
        slab_u[t] = su;
      }
      __syncthreads();  // the LDS slots are reused by the next tile
    }
  }
}

// One block adds each tensor's tiles (combine_tiles, tile_plan.h): one fixed
// order whatever the grid of the moments pass. The guard state is only read:
// on a skipped step the slab is stale and the stats stay what they were.
__global__ __launch_bounds__(kFinThreads) void lamb_finalise_kernel(
    const float* __restrict__ slab_w, const float* __restrict__ slab_u, int T,
    const int4v* __restrict__ tens, int S, const float* __restrict__ st,
    float* __restrict__ stats) {
  if (reinterpret_cast<const int*>(st)[kNonFinite] != 0) return;
  combine_tiles(slab_w, slab_u, T, tens, S,
                [&](int s, const int4v& e, double a, double b) {
                  const float wn = (float)sqrt(a), un = (float)sqrt(b);
                  stats[3 * s + 0] = wn;
                  stats[3 * s + 1] = un;
                  stats[3 * s + 2] =
                      (!e[2] && wn > 0.f && un > 0.f) ? wn / un : 1.f;
                });
}

}  // namespace

#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif

// adam_step (slab == nullptr: one kFused pass) and lamb_step (kMoments, the
// combine, kApply) take the same arguments through the same checks
static void adaptive_step(const at::Tensor* slab, const at::Tensor& p,
                          const at::Tensor& g, const at::Tensor& m,
                          const at::Tensor& v, const at::Tensor& table,
                          const at::Tensor& tens, const at::Tensor& state,
                          const at::Tensor& stats, const at::Tensor& clock,
                          const c10::optional<at::Tensor>& lr_dev, double lr,
                          double b1, double b2, double eps, double wd,
                          double gscale, double max_norm,
                          const c10::optional<at::Tensor>& ema) {
  const PlanDims d = check_plan(p, g, state, table, tens, stats);
  check_flat(m, "exp_avg", p.numel());
  check_flat(v, "exp_avg_sq", p.numel());
  check_f32(clock, "clock", kClkLen);
  TORCH_CHECK(clock.device() == p.device(),
              "the clock must live on the parameters' device");
  TORCH_CHECK(b1 >= 0.0 && b1 < 1.0, "beta1 must be in [0, 1), got ", b1);
  TORCH_CHECK(b2 >= 0.0 && b2 < 1.0, "beta2 must be in [0, 1), got ", b2);
  TORCH_CHECK(eps >= 0.0, "eps must be >= 0, got ", eps);
  const float* lr_ptr = lr_dev.has_value() ? check_dev_scalar(*lr_dev, p)
                                           : nullptr;
  float* e = ema.has_value() ? check_ema(*ema, clock, p).e : nullptr;
  if (slab) check_f32(*slab, "plan slab", 2L * d.T);
  if (d.T == 0) return;
  float* sw = slab ? slab->data_ptr<float>() : nullptr;
  float* su = slab ? sw + d.T : nullptr;

  auto tiles = [&](auto kPass) {
    auto launch = [&](auto kEma) {
      launch256(adam_tiles_kernel<kPass, kEma>, dim3(d.grid), 0,
                p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(),
                v.data_ptr<float>(), p.numel(), int4_rows(table), d.T,
                int4_rows(tens), d.S, state.data_ptr<float>(),
                stats.data_ptr<float>(), clock.data_ptr<float>(), lr_ptr, lr,
                b1, b2, eps, wd, gscale, max_norm, e, sw, su);
    };
    if constexpr (kPass == kMoments)
      launch(std::false_type{});  // writes no w, so no EMA variant
    else
      pick<true, false>(e != nullptr, launch);
  };
  if (!slab) {
    tiles(std::integral_constant<int, kFused>{});
    return;
  }
  tiles(std::integral_constant<int, kMoments>{});
  hipLaunchKernelGGL(lamb_finalise_kernel, dim3(1), dim3(kFinThreads), 0,
                     cur_stream(), sw, su, d.T, int4_rows(tens), d.S,
                     state.data_ptr<float>(), stats.data_ptr<float>());
  tiles(std::integral_constant<int, kApply>{});
}

void adam_step(at::Tensor p, at::Tensor g, at::Tensor m, at::Tensor v,
               at::Tensor table, at::Tensor tens, at::Tensor state,
               at::Tensor stats, at::Tensor clock,
               c10::optional<at::Tensor> lr_dev, double lr, double b1,
               double b2, double eps, double wd, double gscale,
               double max_norm, c10::optional<at::Tensor> ema) {
  adaptive_step(nullptr, p, g, m, v, table, tens, state, stats, clock, lr_dev,
                lr, b1, b2, eps, wd, gscale, max_norm, ema);
}

void lamb_step(at::Tensor p, at::Tensor g, at::Tensor m, at::Tensor v,
               at::Tensor table, at::Tensor tens, at::Tensor slab,
               at::Tensor state, at::Tensor stats, at::Tensor clock,
               c10::optional<at::Tensor> lr_dev, double lr, double b1,
               double b2, double eps, double wd, double gscale,
               double max_norm, c10::optional<at::Tensor> ema) {
  adaptive_step(&slab, p, g, m, v, table, tens, state, stats, clock, lr_dev,
                lr, b1, b2, eps, wd, gscale, max_norm, ema);
}
