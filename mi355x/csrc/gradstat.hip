// Whole-gradient statistics and the SGD step they guard: global-norm
// clipping and dynamic fp16 loss scaling with no host round trip.
//
//   grad_stats        pass 1: per-block sum of squares + non-finite count of
//                     the flat fp32 grad buffer into a slab (<= 2048 entries),
//                     then a one-block finalise that adds the slab in a fixed
//                     order (double) -> {non-finite count, raw norm}
//   sgd_step_guarded  sgd_kernel's arithmetic with the gradient multiplier
//                     taken from the device; writes nothing if the gradient
//                     holds an inf/nan
//   scaler_update     one thread, after the step: dynamic loss-scale update
//                     (GradScaler.step_ok's rules) + last norm/coef for logs
//
// No float atomics and no last-block ticket: the slab is combined by one
// block in one order, so the norm (and with it the clip coefficient) is
// bit-identical from run to run and between DDP ranks that hold the same
// gradient.
//
// Guard state: ONE float32[8] device tensor owned by the Python object
// (amp.DeviceGradScaler, or optim.SGD when it only clips). Integer fields
// hold int32 bit patterns (view(torch.int32) on the Python side).
//
//   [0] scale        loss scale                       (float)
//   [1] inv_scale    1 / scale                        (float)
//   [2] tracker      clean steps since last change    (int32)
//   [3] skipped      steps skipped for inf/nan so far (int32)
//   [4] nonfinite    inf/nan elements, last grad      (int32)  <- grad_stats
//   [5] raw_norm     ||flat_grad||_2 as stored        (float)  <- grad_stats
//   [6] last_norm    norm of the true gradient:
//                    raw_norm * gscale * inv_scale    (float)
//   [7] last_coef    clip coefficient of that step    (float)
//
// grad_stats writes its two results to any float32[2] {count, raw norm};
// optim.SGD hands it state[4:6].
//
//   clock_advance     one thread, after scaler_update: counts the step if it
//                     was applied and looks up what the next one uses
//
// Step clock: ONE float32[4] device tensor owned by the optimizer that has a
// learning-rate schedule or a weight EMA. The update kernels read lr and the
// EMA weight from it, so a captured step follows the schedule with no host
// write, and a step skipped for overflow does not advance it.
//
//   [0] step      applied steps so far                     (int32)
//   [1] lr        table[min(step, T-1)]: the lr the next
//                 step uses                                 (float)
//   [2] ema_omd   1 - d_step, the weight of the new
//                 parameters in the next step's average     (float)
//   [3] reserved  0
//
// d_t = decay, or min(decay, (1 + t) / (10 + t)) with the EMA warm-up, in
// double and rounded once, so the host (which fills the clock for step 0
// and after a checkpoint load) and the CPU fallback agree to the bit. The
// schedule is a float32 table built on the host: no transcendental here.
//
// Elementwise conventions as in elementwise.hip: 16 B/lane loads, grid-stride
// loop, at most 2048 workgroups, scalar tail.
#include "common.h"
#include "guard.h"

#include <climits>
#include <cmath>

namespace {

constexpr int kMaxBlocks = 2048;  // slab: [kMaxBlocks] sumsq + [kMaxBlocks] counts

__global__ __launch_bounds__(256) void grad_stats_kernel(
    const float* __restrict__ g, long n, float* __restrict__ slab_sq,
    int* __restrict__ slab_nf) {
  long i0 = (long)(blockIdx.x * blockDim.x + threadIdx.x) * 4;
  long stride = (long)gridDim.x * blockDim.x * 4;
  float4v acc = {0.f, 0.f, 0.f, 0.f};
  int bad = 0;
  for (long i = i0; i < n; i += stride) {
    if (i + 4 <= n) {
      float4v v = *reinterpret_cast<const float4v*>(g + i);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        acc[k] += v[k] * v[k];
        bad += non_finite(v[k]);
      }
    } else {
      for (long k = i; k < n; ++k) {
        acc[0] += g[k] * g[k];
        bad += non_finite(g[k]);
      }
    }
  }
  float s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s += __shfl_xor(s, off, kWave);
    bad += __shfl_xor(bad, off, kWave);
  }
  __shared__ float ls[4];
  __shared__ int lb[4];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    ls[wave] = s;
    lb[wave] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    slab_sq[blockIdx.x] = (ls[0] + ls[1]) + (ls[2] + ls[3]);
    slab_nf[blockIdx.x] = (lb[0] + lb[1]) + (lb[2] + lb[3]);
  }
}

// one block: slab -> out[0] = non-finite count (int32 bits), out[1] = norm.
// Thread t adds entries t, t+256, ... in double, then a butterfly and four
// LDS slots: one fixed order whatever the grid of pass 1 was doing.
__global__ __launch_bounds__(256) void grad_stats_finalise_kernel(
    const float* __restrict__ slab_sq, const int* __restrict__ slab_nf, int nb,
    float* __restrict__ out) {
  double s = 0.0;
  long long c = 0;
  for (int j = threadIdx.x; j < nb; j += 256) {
    s += (double)slab_sq[j];
    c += slab_nf[j];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s += __shfl_xor(s, off, kWave);
    c += __shfl_xor(c, off, kWave);
  }
  __shared__ double ls[4];
  __shared__ long long lc[4];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    ls[wave] = s;
    lc[wave] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double tot = (ls[0] + ls[1]) + (ls[2] + ls[3]);
    const long long cnt = (lc[0] + lc[1]) + (lc[2] + lc[3]);
    reinterpret_cast<int*>(out)[0] = (int)(cnt > INT_MAX ? INT_MAX : cnt);
    out[1] = (float)sqrt(tot);
  }
}

// lr by value, or read from the device (the clock's lr slot) when lr_dev is
// given. kEma: the weight average e follows w in the same pass, with the
// weight clock[kClkEmaOmd]; e and clock are not touched otherwise.
template <bool kEma>
__global__ void sgd_guarded_kernel(float* __restrict__ p,
                                   const float* __restrict__ g,
                                   float* __restrict__ m, long n,
                                   const float* __restrict__ st,
                                   const float* __restrict__ lr_dev,
                                   float lr_host, float mu, float wd,
                                   float gscale_host, float max_norm,
                                   float* __restrict__ e,
                                   const float* __restrict__ clock) {
  if (reinterpret_cast<const int*>(st)[kNonFinite] != 0) return;  // skipped: no write
  const float gscale = guard_coef(st, gscale_host, max_norm).eff;
  const float lr = lr_dev ? *lr_dev : lr_host;
  float omd = 0.f;
  if constexpr (kEma) omd = clock[kClkEmaOmd];
  long i0 = (long)(blockIdx.x * blockDim.x + threadIdx.x) * 4;
  long stride = (long)gridDim.x * blockDim.x * 4;
  for (long i = i0; i < n; i += stride) {
    if (i + 4 <= n) {
      float4v vg = *reinterpret_cast<const float4v*>(g + i);
      float4v vp = *reinterpret_cast<const float4v*>(p + i);
      float4v vm = *reinterpret_cast<const float4v*>(m + i);
      float4v ve;
      if constexpr (kEma) ve = *reinterpret_cast<const float4v*>(e + i);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float gr = vg[k] * gscale + wd * vp[k];
        vm[k] = mu * vm[k] + gr;
        vp[k] -= lr * vm[k];
        if constexpr (kEma) {
          float a = ve[k];
          ema_elem(a, vp[k], omd);
          ve[k] = a;
        }
      }
      *reinterpret_cast<float4v*>(m + i) = vm;
      *reinterpret_cast<float4v*>(p + i) = vp;
      if constexpr (kEma) *reinterpret_cast<float4v*>(e + i) = ve;
    } else {
      for (long k = i; k < n; ++k) {
        float gr = g[k] * gscale + wd * p[k];
        m[k] = mu * m[k] + gr;
        p[k] -= lr * m[k];
        if constexpr (kEma) ema_elem(e[k], p[k], omd);
      }
    }
  }
}

// One thread, launched after scaler_update on the same stream. st may be
// null (no guard: every step counts). A skipped step leaves the clock alone.
__global__ void clock_advance_kernel(float* ck, const float* st,
                                     const float* __restrict__ table, int T,
                                     double decay, int warmup) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (st && reinterpret_cast<const int*>(st)[kNonFinite] != 0) return;
  int* cki = reinterpret_cast<int*>(ck);
  const int prev = cki[kClkStep];
  const int t = prev < INT_MAX ? max(prev, -1) + 1 : INT_MAX;
  double d = decay;
  if (warmup) d = fmin(decay, (1.0 + (double)t) / (10.0 + (double)t));
  cki[kClkStep] = t;
  ck[kClkLr] = table[min(t, T - 1)];
  ck[kClkEmaOmd] = (float)(1.0 - d);
}

// One thread, launched after the guarded step on the same stream, so no SGD
// block still reads the scale it rewrites. interval <= 0: no dynamic scale
// (clip-only state), only the skip counter and the log fields move.
__global__ void scaler_update_kernel(float* st, float gscale, float max_norm,
                                     float growth, float backoff,
                                     int interval) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const GuardCoef c = guard_coef(st, gscale, max_norm);
  int* sti = reinterpret_cast<int*>(st);
  float scale = st[kScale];
  int tracker = sti[kTracker];
  int skipped = sti[kSkipped];
  if (sti[kNonFinite] != 0) {
    ++skipped;
    if (interval > 0) {
      scale *= backoff;
      tracker = 0;
    }
  } else if (interval > 0) {
    ++tracker;
    if (tracker >= interval) {
      scale *= growth;
      tracker = 0;
    }
  }
  st[kScale] = scale;
  st[kInvScale] = 1.f / scale;
  sti[kTracker] = tracker;
  sti[kSkipped] = skipped;
  st[kLastNorm] = c.norm;
  st[kLastCoef] = c.coef;
}

inline int gs_grid(long n) {
  long blocks = cdiv_l(n, (long)256 * 4);
  return (int)std::max<long>(1, std::min<long>(blocks, kMaxBlocks));
}

}  // namespace

void grad_stats(at::Tensor g, at::Tensor slab, at::Tensor out) {
  check_f32(g, "g", 0);
  check_f32(slab, "slab", 2 * kMaxBlocks);
  check_f32(out, "out", 2);
  const long n = g.numel();
  const int nb = gs_grid(n);
  float* sq = slab.data_ptr<float>();
  int* nf = reinterpret_cast<int*>(sq + kMaxBlocks);
  hipLaunchKernelGGL(grad_stats_kernel, dim3(nb), dim3(256), 0, cur_stream(),
                     g.data_ptr<float>(), n, sq, nf);
  hipLaunchKernelGGL(grad_stats_finalise_kernel, dim3(1), dim3(256), 0,
                     cur_stream(), sq, nf, nb, out.data_ptr<float>());
}

void sgd_step_guarded(at::Tensor p, at::Tensor g, at::Tensor m,
                      at::Tensor state, c10::optional<at::Tensor> lr_dev,
                      double lr, double mu, double wd, double gscale,
                      double max_norm, c10::optional<at::Tensor> ema,
                      c10::optional<at::Tensor> clock) {
  check_f32(p, "p", 0);
  check_f32(g, "g", 0);
  check_f32(m, "m", 0);
  check_f32(state, "state", kStateLen);
  const long n = p.numel();
  TORCH_CHECK(g.numel() == n && m.numel() == n,
              "p, g and m must have the same number of elements");
  const float* lr_ptr = lr_dev.has_value() ? check_dev_scalar(*lr_dev, p)
                                           : nullptr;
  const dim3 grid(gs_grid(n)), block(256);
  if (ema.has_value()) {
    const EmaArgs a = check_ema(*ema, clock, p);
    hipLaunchKernelGGL(sgd_guarded_kernel<true>, grid, block, 0, cur_stream(),
                       p.data_ptr<float>(), g.data_ptr<float>(),
                       m.data_ptr<float>(), n, state.data_ptr<float>(), lr_ptr,
                       (float)lr, (float)mu, (float)wd, (float)gscale,
                       (float)max_norm, a.e, a.clock);
    return;
  }
  hipLaunchKernelGGL(sgd_guarded_kernel<false>, grid, block, 0, cur_stream(),
                     p.data_ptr<float>(), g.data_ptr<float>(),
                     m.data_ptr<float>(), n, state.data_ptr<float>(), lr_ptr,
                     (float)lr, (float)mu, (float)wd, (float)gscale,
                     (float)max_norm, (float*)nullptr, (const float*)nullptr);
}

void clock_advance(at::Tensor clock, c10::optional<at::Tensor> state,
                   at::Tensor table, double decay, bool warmup) {
  check_f32(clock, "clock", kClkLen);
  check_f32(table, "schedule table", 1);
  TORCH_CHECK(table.numel() < (long)INT_MAX, "schedule table too long");
  TORCH_CHECK(table.device() == clock.device(),
              "the schedule table must live on the clock's device");
  const float* st = nullptr;
  if (state.has_value()) {
    check_f32(*state, "state", kStateLen);
    TORCH_CHECK(state->device() == clock.device(),
                "the guard state must live on the clock's device");
    st = state->data_ptr<float>();
  }
  hipLaunchKernelGGL(clock_advance_kernel, dim3(1), dim3(1), 0, cur_stream(),
                     clock.data_ptr<float>(), st, table.data_ptr<float>(),
                     (int)table.numel(), decay, (int)warmup);
}

void scaler_update(at::Tensor state, double gscale, double max_norm,
                   double growth, double backoff, long interval) {
  check_f32(state, "state", kStateLen);
  hipLaunchKernelGGL(scaler_update_kernel, dim3(1), dim3(1), 0, cur_stream(),
                     state.data_ptr<float>(), (float)gscale, (float)max_norm,
                     (float)growth, (float)backoff,
                     (int)std::min<long>(interval, INT_MAX));
}
