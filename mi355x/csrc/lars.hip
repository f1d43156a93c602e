// LARS (layer-wise adaptive rate scaling) over the flat fp32 buffers: a
// per-tensor reduction that respects tensor boundaries inside the flat
// buffer, and an update kernel with one multiplier per tensor.
//
//   lars_stats   pass 1: per TILE sum of squares of w, of g and the
//                non-finite count of g into a slab; then one finalise block
//                that adds each tensor's tiles in tile order (double), the
//                per-tensor g sums in tensor order (double) -> state[4:6] as
//                grad_stats leaves them, and {||w_s||, raw ||g_s||, trust_s}
//                per tensor into stats[S][3]
//   lars_step    gr = g*eff + wd_s*w; m = mu*m + trust_s*gr; w -= lr*m,
//                eff from the guard state (guard.h); writes nothing if the
//                gradient holds an inf/nan. lr by value or read from a 0-d
//                device tensor, so a captured step follows a schedule. With
//                an EMA buffer, e += omd*(w - e) in the same pass, omd from
//                the step clock (gradstat.hip).
//
// The plan (built once on the host, mi355x.ops.lars_plan) cuts the flat
// buffers into tiles of at most kTile elements that never cross a tensor
// boundary:
//   table[T][4] int32   {start element, length, tensor, 0}
//   tens[S][4]  int32   {first tile, one past last tile, excluded, 0}
// Tensors start anywhere (61 of ResNet-18's 62 at an offset that is no
// multiple of 4), so a tile is a scalar head up to 16-byte alignment, a
// 16 B/lane body and a scalar tail. The buffers themselves must be 16-byte
// aligned.
//
// The plan's constants, the tile decode, the per-tensor combine and the
// argument checks are in tile_plan.h (adam.hip walks the same plan); the
// block sum of pass 1 is reduce.h's, as in gradstat.hip.
//
// As in gradstat.hip: no float atomics, no last-block ticket. A tile's
// partial is formed by one block in one order and pass 1 only strides over
// tiles, so every norm and trust ratio is bit-identical from run to run,
// whatever the grid, and between DDP ranks that hold the same gradient.
#include "common.h"
#include "guard.h"
#include "tile_plan.h"

#include <climits>
#include <cmath>
#include <cstdint>

namespace {

__global__ __launch_bounds__(256) void lars_partials_kernel(
    const float* __restrict__ w, const float* __restrict__ g, long n,
    const int4v* __restrict__ table, int T, int S, float* __restrict__ slab_w,
    float* __restrict__ slab_g, int* __restrict__ slab_nf) {
  const int tid = threadIdx.x;
  for (int t = blockIdx.x; t < T; t += gridDim.x) {
    const Tile q = load_tile(table, t, n, S);
    float4v aw = {0.f, 0.f, 0.f, 0.f}, ag = {0.f, 0.f, 0.f, 0.f};
    // a tile that cannot be read makes the step skip instead of half-count
    int bad = q.ok ? 0 : (tid == 0);
    if (q.ok) {
      const float* wt = w + q.start;
      const float* gt = g + q.start;
      if (tid < q.head) {
        const float a = wt[tid], b = gt[tid];
        aw[0] += a * a;
        ag[0] += b * b;
        bad += non_finite(b);
      }
      const float4v* wv = reinterpret_cast<const float4v*>(wt + q.head);
      const float4v* gv = reinterpret_cast<const float4v*>(gt + q.head);
#pragma unroll
      for (int k = 0; k < kVecs; ++k) {
        const int v = tid + k * 256;
        if (v < q.nvec) {
          const float4v a = wv[v], b = gv[v];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            aw[j] += a[j] * a[j];
            ag[j] += b[j] * b[j];
            bad += non_finite(b[j]);
          }
        }
      }
      if (tid < q.tail) {
        const int i = q.head + 4 * q.nvec + tid;
        const float a = wt[i], b = gt[i];
        aw[0] += a * a;
        ag[0] += b * b;
        bad += non_finite(b);
      }
    }
    float sw = sum4(aw[0], aw[1], aw[2], aw[3]);
    float sg = sum4(ag[0], ag[1], ag[2], ag[3]);
    block_sum256(sw, sg, bad);
    if (tid == 0) {
      slab_w[t] = sw;
      slab_g[t] = sg;
      slab_nf[t] = bad;
    }
    __syncthreads();  // the LDS slots are reused by the next tile
  }
}

// trust_s with every product, sum and quotient rounded on its own, so the
// CPU fallback (one torch op per line) follows it
DEV_INLINE float trust_ratio(float wn, float gn_raw, float eff, float wd,
                             float eta, float eps) {
#pragma clang fp contract(off)
  const float gn = gn_raw * eff;
  if (!(wn > 0.f && gn > 0.f)) return 1.f;
  const float decay = wd * wn;
  const float den = (gn + decay) + eps;
  const float num = eta * wn;
  return num / den;
}

// One block. combine_tiles (tile_plan.h) adds each tensor's tiles, then wave
// 0 adds the per-tensor g sums the same way: lane l takes tensors l, l+64,
// ... in double, then a butterfly. One fixed order whatever pass 1's grid.
__global__ __launch_bounds__(kFinThreads) void lars_finalise_kernel(
    const float* __restrict__ slab_w, const float* __restrict__ slab_g,
    const int* __restrict__ slab_nf, int T, const int4v* __restrict__ tens,
    int S, float* __restrict__ st, float* __restrict__ stats, float gscale,
    float max_norm, float wd, float eta, float eps) {
  extern __shared__ double lsum[];  // [S] sums of w^2, then [S] of g^2
  __shared__ long long lc[kFinWaves];
  __shared__ float raw_norm;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  double* sum_w = lsum;
  double* sum_g = lsum + S;

  combine_tiles(slab_w, slab_g, T, tens, S,
                [&](int s, const int4v&, double a, double b) {
                  sum_w[s] = a;
                  sum_g[s] = b;
                });
  long long c = 0;
  for (int t = tid; t < T; t += kFinThreads) c += slab_nf[t];
  c = wave_sum(c);
  if (lane == 0) lc[wave] = c;
  __syncthreads();

  if (wave == 0) {
    double tot = 0.0;
    for (int s = lane; s < S; s += kWave) tot += sum_g[s];
    tot = wave_sum(tot);
    if (lane == 0) {
      long long cnt = 0;
      for (int k = 0; k < kFinWaves; ++k) cnt += lc[k];
      const float r = (float)sqrt(tot);
      reinterpret_cast<int*>(st)[kNonFinite] =
          (int)(cnt > INT_MAX ? INT_MAX : cnt);
      st[kRawNorm] = r;
      raw_norm = r;
    }
  }
  __syncthreads();

  const float eff =
      guard_coef_of(raw_norm, st[kInvScale], gscale, max_norm).eff;
  for (int s = tid; s < S; s += kFinThreads) {
    const float wn = (float)sqrt(sum_w[s]);
    const float gn = (float)sqrt(sum_g[s]);
    stats[3 * s + 0] = wn;
    stats[3 * s + 1] = gn;
    stats[3 * s + 2] =
        tens[s][2] ? 1.f : trust_ratio(wn, gn, eff, wd, eta, eps);
  }
}

DEV_INLINE void lars_elem(float& w, float g, float& m, float eff, float wd,
                          float trust, float mu, float lr) {
  // the roundings spelled out, not left to contraction: with trust == 1
  // these are the operations of sgd_kernel's 16-byte path
#pragma clang fp contract(off)
  const float gr = fmaf(g, eff, wd * w);
  m = fmaf(mu, m, trust * gr);
  w = fmaf(-lr, m, w);
}

// kEma: the weight average e (w's layout and alignment) follows w in the
// same pass with the weight clock[kClkEmaOmd]: head, body and tail as for w.
// e and clock are not touched otherwise.
template <bool kEma>
__global__ __launch_bounds__(256) void lars_update_kernel(
    float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m,
    long n, const int4v* __restrict__ table, int T,
    const int4v* __restrict__ tens, int S, const float* __restrict__ st,
    const float* __restrict__ stats, const float* __restrict__ lr_dev,
    float lr_host, float mu, float wd_host, float gscale_host,
    float max_norm, float* __restrict__ e, const float* __restrict__ clock) {
  if (reinterpret_cast<const int*>(st)[kNonFinite] != 0) return;  // skipped: no write
  const float eff = guard_coef(st, gscale_host, max_norm).eff;
  const float lr = lr_dev ? *lr_dev : lr_host;
  float omd = 0.f;
  if constexpr (kEma) omd = clock[kClkEmaOmd];
  const int tid = threadIdx.x;
  for (int t = blockIdx.x; t < T; t += gridDim.x) {
    const Tile q = load_tile(table, t, n, S);
    if (!q.ok) continue;
    const float trust = stats[3 * q.tensor + 2];
    const float wd = tens[q.tensor][2] ? 0.f : wd_host;
    float* wt = w + q.start;
    const float* gt = g + q.start;
    float* mt = m + q.start;
    float* et = nullptr;
    if constexpr (kEma) et = e + q.start;
    if (tid < q.head) {
      lars_elem(wt[tid], gt[tid], mt[tid], eff, wd, trust, mu, lr);
      if constexpr (kEma) ema_elem(et[tid], wt[tid], omd);
    }
    float4v* wv = reinterpret_cast<float4v*>(wt + q.head);
    const float4v* gv = reinterpret_cast<const float4v*>(gt + q.head);
    float4v* mv = reinterpret_cast<float4v*>(mt + q.head);
    float4v* ev = nullptr;
    if constexpr (kEma) ev = reinterpret_cast<float4v*>(et + q.head);
    float4v vw[kVecs], vg[kVecs], vm[kVecs], ve[kVecs];
#pragma unroll
    for (int k = 0; k < kVecs; ++k) {
      const int v = tid + k * 256;
      if (v < q.nvec) {
        vg[k] = gv[v];
        vw[k] = wv[v];
        vm[k] = mv[v];
        if constexpr (kEma) ve[k] = ev[v];
      }
    }
#pragma unroll
    for (int k = 0; k < kVecs; ++k) {
      const int v = tid + k * 256;
      if (v < q.nvec) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float a = vw[k][j], b = vm[k][j];
          lars_elem(a, vg[k][j], b, eff, wd, trust, mu, lr);
          vw[k][j] = a;
          vm[k][j] = b;
          if constexpr (kEma) {
            float c = ve[k][j];
            ema_elem(c, a, omd);
            ve[k][j] = c;
          }
        }
        mv[v] = vm[k];
        wv[v] = vw[k];
        if constexpr (kEma) ev[v] = ve[k];
      }
    }
    if (tid < q.tail) {
      const int i = q.head + 4 * q.nvec + tid;
      lars_elem(wt[i], gt[i], mt[i], eff, wd, trust, mu, lr);
      if constexpr (kEma) ema_elem(et[i], wt[i], omd);
    }
  }
}

}  // namespace

void lars_stats(at::Tensor p, at::Tensor g, at::Tensor table, at::Tensor tens,
                at::Tensor slab, at::Tensor state, at::Tensor stats,
                double gscale, double max_norm, double wd, double eta,
                double eps) {
  const PlanDims d = check_plan(p, g, state, table, tens, stats);
  check_f32(slab, "plan slab", 3L * d.T);
  float* sw = slab.data_ptr<float>();
  float* sg = sw + d.T;
  int* nf = reinterpret_cast<int*>(sg + d.T);
  if (d.T > 0)
    launch256(lars_partials_kernel, dim3(d.grid), 0, p.data_ptr<float>(),
              g.data_ptr<float>(), p.numel(), int4_rows(table), d.T, d.S, sw,
              sg, nf);
  hipLaunchKernelGGL(lars_finalise_kernel, dim3(1), dim3(kFinThreads),
                     2 * d.S * sizeof(double), cur_stream(), sw, sg, nf, d.T,
                     int4_rows(tens), d.S, state.data_ptr<float>(),
                     stats.data_ptr<float>(),
                     (float)gscale, (float)max_norm, (float)wd, (float)eta,
                     (float)eps);
}

void lars_step(at::Tensor p, at::Tensor g, at::Tensor m, at::Tensor table,
               at::Tensor tens, at::Tensor state, at::Tensor stats,
               c10::optional<at::Tensor> lr_dev, double lr, double mu,
               double wd, double gscale, double max_norm,
               c10::optional<at::Tensor> ema,
               c10::optional<at::Tensor> clock) {
  const PlanDims d = check_plan(p, g, state, table, tens, stats);
  check_flat(m, "m", p.numel());
  const float* lr_ptr = lr_dev.has_value() ? check_dev_scalar(*lr_dev, p)
                                           : nullptr;
  EmaArgs a = {nullptr, nullptr};
  if (ema.has_value()) a = check_ema(*ema, clock, p);
  if (d.T == 0) return;
  pick<true, false>(ema.has_value(), [&](auto kEma) {
    launch256(lars_update_kernel<kEma>, dim3(d.grid), 0, p.data_ptr<float>(),
              g.data_ptr<float>(), m.data_ptr<float>(), p.numel(),
              int4_rows(table), d.T, int4_rows(tens), d.S,
              state.data_ptr<float>(), stats.data_ptr<float>(), lr_ptr, lr, mu,
              wd, gscale, max_norm, a.e, a.clock);
  });
}
