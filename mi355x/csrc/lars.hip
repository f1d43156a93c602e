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
// As in gradstat.hip: no float atomics, no last-block ticket. A tile's
// partial is formed by one block in one order and pass 1 only strides over
// tiles, so every norm and trust ratio is bit-identical from run to run,
// whatever the grid, and between DDP ranks that hold the same gradient.
#include "common.h"
#include "guard.h"

#include <climits>
#include <cmath>
#include <cstdint>

namespace {

constexpr int kTile = 4096;
constexpr int kVecs = 4;  // 16-byte vectors per thread and tile
static_assert(kTile == 256 * 4 * kVecs, "a tile is one sweep of a block");
constexpr int kMaxGrid = 2048;
constexpr int kMaxTensors = 2048;  // finalise keeps 16 B of LDS per tensor
constexpr int kFinThreads = 1024;
constexpr int kFinWaves = kFinThreads / kWave;

struct Tile {
  const int ok;
  const long start;
  const int head, nvec, tail, tensor;
};

// A tile outside the buffers (a table that does not belong to them) is
// never touched: ok == 0.
DEV_INLINE Tile load_tile(const int4v* __restrict__ table, int t, long n,
                          int S) {
  const int4v e = table[t];
  const int ok = e[0] >= 0 && e[1] >= 0 && e[1] <= kTile &&
                 (long)e[0] + e[1] <= n && e[2] >= 0 && e[2] < S;
  const int head = min((4 - (e[0] & 3)) & 3, e[1]);
  const int nvec = (e[1] - head) >> 2;
  return {ok, (long)e[0], head, nvec, e[1] - head - 4 * nvec, e[2]};
}

__global__ __launch_bounds__(256) void lars_partials_kernel(
    const float* __restrict__ w, const float* __restrict__ g, long n,
    const int4v* __restrict__ table, int T, int S, float* __restrict__ slab_w,
    float* __restrict__ slab_g, int* __restrict__ slab_nf) {
  __shared__ float lw[4], lg[4];
  __shared__ int lb[4];
  const int tid = threadIdx.x, wave = tid >> 6;
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
    float sw = (aw[0] + aw[1]) + (aw[2] + aw[3]);
    float sg = (ag[0] + ag[1]) + (ag[2] + ag[3]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      sw += __shfl_xor(sw, off, kWave);
      sg += __shfl_xor(sg, off, kWave);
      bad += __shfl_xor(bad, off, kWave);
    }
    if ((tid & 63) == 0) {
      lw[wave] = sw;
      lg[wave] = sg;
      lb[wave] = bad;
    }
    __syncthreads();
    if (tid == 0) {
      slab_w[t] = (lw[0] + lw[1]) + (lw[2] + lw[3]);
      slab_g[t] = (lg[0] + lg[1]) + (lg[2] + lg[3]);
      slab_nf[t] = (lb[0] + lb[1]) + (lb[2] + lb[3]);
    }
    __syncthreads();  // the LDS slots are reused by the next tile
  }
}

DEV_INLINE double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
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

// One block. Wave v owns tensors v, v+16, ...: lane l adds the tensor's
// tiles l, l+64, ... in double, then a butterfly. Wave 0 then adds the
// per-tensor g sums the same way. One fixed order whatever pass 1's grid.
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

  for (int s = wave; s < S; s += kFinWaves) {
    const int4v e = tens[s];
    const int t0 = max(e[0], 0), t1 = min(e[1], T);
    double a = 0.0, b = 0.0;
    for (int t = t0 + lane; t < t1; t += kWave) {
      a += (double)slab_w[t];
      b += (double)slab_g[t];
    }
    a = wave_sum(a);
    b = wave_sum(b);
    if (lane == 0) {
      sum_w[s] = a;
      sum_g[s] = b;
    }
  }
  long long c = 0;
  for (int t = tid; t < T; t += kFinThreads) c += slab_nf[t];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, kWave);
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

inline void check_i32x4(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == at::kInt, name, " must be int32");
  TORCH_CHECK(t.dim() == 2 && t.size(1) == 4, name, " must be [rows, 4]");
}

inline void check_flat(const at::Tensor& t, const char* name, long n) {
  check_f32(t, name, 0);
  TORCH_CHECK(t.numel() == n, name, " must have ", n,
              " elements like the parameters");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr<float>()) % 16 == 0,
              name, " must start at a 16-byte aligned address");
}

struct PlanDims {
  int T, S, grid;
};

inline PlanDims check_plan(const at::Tensor& table, const at::Tensor& tens,
                           const at::Tensor& stats, long n) {
  check_i32x4(table, "plan table");
  check_i32x4(tens, "plan tensor table");
  const long T = table.size(0), S = tens.size(0);
  TORCH_CHECK(n < (long)INT_MAX, "flat buffers of 2^31 elements or more");
  TORCH_CHECK(S >= 1 && S <= kMaxTensors, "plan must hold 1..", kMaxTensors,
              " tensors, got ", S);
  TORCH_CHECK(T < (long)INT_MAX, "too many tiles");
  check_f32(stats, "plan stats", 0);
  TORCH_CHECK(stats.dim() == 2 && stats.size(0) == S && stats.size(1) == 3,
              "plan stats must be [", S, ", 3]");
  return {(int)T, (int)S, (int)std::max<long>(1, std::min<long>(T, kMaxGrid))};
}

}  // namespace

void lars_stats(at::Tensor p, at::Tensor g, at::Tensor table, at::Tensor tens,
                at::Tensor slab, at::Tensor state, at::Tensor stats,
                double gscale, double max_norm, double wd, double eta,
                double eps) {
  const long n = p.numel();
  check_flat(p, "p", n);
  check_flat(g, "g", n);
  check_f32(state, "state", kStateLen);
  const PlanDims d = check_plan(table, tens, stats, n);
  check_f32(slab, "plan slab", 3L * d.T);
  float* sw = slab.data_ptr<float>();
  float* sg = sw + d.T;
  int* nf = reinterpret_cast<int*>(sg + d.T);
  const int4v* tb = reinterpret_cast<const int4v*>(table.data_ptr<int>());
  const int4v* tn = reinterpret_cast<const int4v*>(tens.data_ptr<int>());
  if (d.T > 0)
    hipLaunchKernelGGL(lars_partials_kernel, dim3(d.grid), dim3(256), 0,
                       cur_stream(), p.data_ptr<float>(), g.data_ptr<float>(),
                       n, tb, d.T, d.S, sw, sg, nf);
  hipLaunchKernelGGL(lars_finalise_kernel, dim3(1), dim3(kFinThreads),
                     2 * d.S * sizeof(double), cur_stream(), sw, sg, nf, d.T,
                     tn, d.S, state.data_ptr<float>(), stats.data_ptr<float>(),
                     (float)gscale, (float)max_norm, (float)wd, (float)eta,
                     (float)eps);
}

void lars_step(at::Tensor p, at::Tensor g, at::Tensor m, at::Tensor table,
               at::Tensor tens, at::Tensor state, at::Tensor stats,
               c10::optional<at::Tensor> lr_dev, double lr, double mu,
               double wd, double gscale, double max_norm,
               c10::optional<at::Tensor> ema,
               c10::optional<at::Tensor> clock) {
  const long n = p.numel();
  check_flat(p, "p", n);
  check_flat(g, "g", n);
  check_flat(m, "m", n);
  check_f32(state, "state", kStateLen);
  const PlanDims d = check_plan(table, tens, stats, n);
  const float* lr_ptr = lr_dev.has_value() ? check_dev_scalar(*lr_dev, p)
                                           : nullptr;
  EmaArgs a = {nullptr, nullptr};
  if (ema.has_value()) a = check_ema(*ema, clock, p);
  if (d.T == 0) return;
#define LARS_UPDATE(EMA)                                                     \
  hipLaunchKernelGGL(                                                        \
      lars_update_kernel<EMA>, dim3(d.grid), dim3(256), 0, cur_stream(),     \
      p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(), n,      \
      reinterpret_cast<const int4v*>(table.data_ptr<int>()), d.T,            \
      reinterpret_cast<const int4v*>(tens.data_ptr<int>()), d.S,             \
      state.data_ptr<float>(), stats.data_ptr<float>(), lr_ptr, (float)lr,   \
      (float)mu, (float)wd, (float)gscale, (float)max_norm, a.e, a.clock)
  if (ema.has_value())
    LARS_UPDATE(true);
  else
    LARS_UPDATE(false);
#undef LARS_UPDATE
}
