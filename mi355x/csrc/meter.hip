// Device-side loss / top-k / confusion meter: what a training or evaluation
// loop wants to log about a batch of logits, accumulated on the device with
// no host read (metrics.DeviceMeter reads the state when a line is printed).
//
//   meter_rows      pass 1: per row lse, nll, argmax and the label's rank;
//                   per-block partials {nll sum, correct@1, correct@k, bad}
//                   into a slab (<= 2048 entries), confusion counts into the
//                   [C,C] int64 matrix
//   meter_finalise  one block: adds the slab in one fixed order (the nll sums
//                   in double) and adds the result into the state
//
// No float atomics and no last-block ticket (the rule at the top of
// gradstat.hip): the loss sum is bit-identical from run to run. The only
// atomics are integer adds into the confusion matrix, which are exact in any
// order.
//
// Meter state: ONE int64[8] device tensor owned by metrics.DeviceMeter.
//
//   [0] rows        rows seen
//   [1] correct1    good rows whose label ranks first
//   [2] correctk    good rows whose label ranks among the first k
//   [3] bad         rows with a label outside [0,C) or a non-finite lse
//   [4] loss_sum    sum of the rows' nll, or of loss*B for an update that was
//                   handed its loss: a float64 bit pattern
//                   (state[4:5].view(torch.float64) on the Python side)
//   [5] updates     meter_update calls
//   [6..7]          0
//
// Slab: int64[4 * 2048]: per block the nll sum (float64 bits), then the
// three counts, each array 2048 long.
//
// Row definitions (the plain-torch twin in ops/functional.py makes the same
// decisions, so counts and matrix agree with it to the bit):
//   t    = y_a, or with a mix target lam >= 0.5 ? y_a : y_b
//   lse, nll = lse - z_t in ce_fwd_kernel's arithmetic (fp32, __expf/__logf,
//          the same reduction tree, so a row's nll equals that kernel's)
//   pred = first index of the row maximum (torch.argmax's tie rule)
//   rank = #{c : z_c > z_t} + #{c < t : z_c == z_t}; top-k is rank < k
//   bad  = t outside [0,C) or lse not finite; a bad label is never an
//          address; a bad row counts in rows and bad and nowhere else
//
// Row packing: a row is worked on by a group of G lanes, 256/G rows per
// block pass. G = 16 for C <= 16 (CIFAR's C = 10 keeps 10 of 16 lanes busy,
// four rows per wave, 16 per block; width-16 shuffles), G = 64 (one wave per
// row, lane loop above 64 columns) otherwise. Both variants: no scratch, no
// LDS beyond the partial slots (+ the confusion tile), 16-bit scalar loads
// since row starts are 2*C bytes apart. The one-wave-per-row layout at
// C = 10 is kept selectable (pack = 64) for the A/B in
// benchmarks/meter_bench.py; results: profiles/r12_meter.md.
#include "common.h"
#include "guard.h"

#include <climits>
#include <cstdint>

namespace {

constexpr int kMaxBlocks = 2048;
constexpr int kTileMaxC = 64;  // confusion counted in LDS up to here (16 KB)

enum { kRows = 0, kCorrect1, kCorrectK, kBad, kLossSum, kUpdates, kMeterLen = 8 };

// kConf: 0 no matrix, 1 int32 LDS tile per block (C <= 64), 2 one global
// 64-bit atomic per good row.
template <typename T16, int G, int kConf>
__global__ __launch_bounds__(256) void meter_rows_kernel(
    const T16* __restrict__ logits, const long* __restrict__ ya,
    const long* __restrict__ yb, const float* __restrict__ lam, int B, int C,
    int k, long long* __restrict__ slab,
    unsigned long long* __restrict__ conf) {
  constexpr int kRowsPerBlock = 256 / G;
  extern __shared__ int tile[];  // [C*C] when kConf == 1
  __shared__ double l_nll[kRowsPerBlock];
  __shared__ int l_cnt[3][kRowsPerBlock];

  if constexpr (kConf == 1) {
    for (int i = threadIdx.x; i < C * C; i += 256) tile[i] = 0;
    __syncthreads();
  }

  const int grp = threadIdx.x / G;
  const int gl = threadIdx.x % G;
  double nll_sum = 0.0;
  int c1 = 0, ck = 0, bad = 0;

  // block-uniform trip count: every lane takes part in the shuffles
  for (long r0 = (long)blockIdx.x * kRowsPerBlock; r0 < B;
       r0 += (long)gridDim.x * kRowsPerBlock) {
    const long b = r0 + grp;
    const bool live = b < B;
    const T16* row = logits + (live ? b : 0) * (long)C;
    long t = -1;
    if (live) {
      t = ya[b];
      if (yb && lam && !(lam[b] >= 0.5f)) t = yb[b];
    }
    const bool t_ok = t >= 0 && t < C;
    const float zt = t_ok ? F16<T16>::to_f32(row[t]) : 0.f;

    // pass 1: maximum and its first index
    float mx = -3.4e38f;
    int arg = INT_MAX;
    if (live) {
      for (int c = gl; c < C; c += G) {
        const float z = F16<T16>::to_f32(row[c]);
        if (z > mx) {
          mx = z;
          arg = c;
        }
      }
    }
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) {
      const float om = __shfl_xor(mx, off, G);
      const int oa = __shfl_xor(arg, off, G);
      if (om > mx || (om == mx && oa < arg)) {
        mx = om;
        arg = oa;
      }
    }
    // pass 2: sum of exponentials and the label's rank
    float s = 0.f;
    int rank = 0;
    if (live) {
      for (int c = gl; c < C; c += G) {
        const float z = F16<T16>::to_f32(row[c]);
        s += __expf(z - mx);
        rank += (z > zt || (z == zt && c < t)) ? 1 : 0;
      }
    }
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) {
      s += __shfl_down(s, off, G);
      rank += __shfl_down(rank, off, G);
    }
    if (gl == 0 && live) {
      const float l = mx + __logf(s);
      const bool good = t_ok && !non_finite(l);
      if (good) {
        nll_sum += (double)(l - zt);
        c1 += rank == 0;
        ck += rank < k;
        if constexpr (kConf != 0) {
          if (arg < C) {  // always, for a finite lse
            const long cell = t * C + arg;
            if constexpr (kConf == 1)
              atomicAdd(&tile[cell], 1);
            else
              atomicAdd(&conf[cell], 1ull);
          }
        }
      } else {
        ++bad;
      }
    }
  }

  if (gl == 0) {
    l_nll[grp] = nll_sum;
    l_cnt[0][grp] = c1;
    l_cnt[1][grp] = ck;
    l_cnt[2][grp] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    // the groups in order: one fixed order for the double sum
    double n = l_nll[0];
    long long a = l_cnt[0][0], bk = l_cnt[1][0], bd = l_cnt[2][0];
    for (int j = 1; j < kRowsPerBlock; ++j) {
      n += l_nll[j];
      a += l_cnt[0][j];
      bk += l_cnt[1][j];
      bd += l_cnt[2][j];
    }
    slab[blockIdx.x] = __double_as_longlong(n);
    slab[kMaxBlocks + blockIdx.x] = a;
    slab[2 * kMaxBlocks + blockIdx.x] = bk;
    slab[3 * kMaxBlocks + blockIdx.x] = bd;
  }
  if constexpr (kConf == 1) {
    for (int i = threadIdx.x; i < C * C; i += 256) {
      const int v = tile[i];
      if (v != 0) atomicAdd(&conf[i], (unsigned long long)v);
    }
  }
}

// one block: slab -> state. Thread t adds entries t, t+256, ... (the nll sums
// in double), then a butterfly and four LDS slots, as
// grad_stats_finalise_kernel. With `loss` (0-d float32, read here) the loss
// sum takes (double)loss * B in place of the rows' nll.
__global__ __launch_bounds__(256) void meter_finalise_kernel(
    const long long* __restrict__ slab, int nb, int B,
    const float* __restrict__ loss, long long* __restrict__ state) {
  double s = 0.0;
  long long a = 0, bk = 0, bd = 0;
  for (int j = threadIdx.x; j < nb; j += 256) {
    s += __longlong_as_double(slab[j]);
    a += slab[kMaxBlocks + j];
    bk += slab[2 * kMaxBlocks + j];
    bd += slab[3 * kMaxBlocks + j];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s += __shfl_xor(s, off, kWave);
    a += __shfl_xor(a, off, kWave);
    bk += __shfl_xor(bk, off, kWave);
    bd += __shfl_xor(bd, off, kWave);
  }
  __shared__ double ls[4];
  __shared__ long long lc[3][4];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    ls[wave] = s;
    lc[0][wave] = a;
    lc[1][wave] = bk;
    lc[2][wave] = bd;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double tot = (ls[0] + ls[1]) + (ls[2] + ls[3]);
    state[kRows] += B;
    state[kCorrect1] += (lc[0][0] + lc[0][1]) + (lc[0][2] + lc[0][3]);
    state[kCorrectK] += (lc[1][0] + lc[1][1]) + (lc[1][2] + lc[1][3]);
    state[kBad] += (lc[2][0] + lc[2][1]) + (lc[2][2] + lc[2][3]);
    const double add = loss ? (double)*loss * (double)B : tot;
    state[kLossSum] =
        __double_as_longlong(__longlong_as_double(state[kLossSum]) + add);
    state[kUpdates] += 1;
  }
}

void check_i64(const at::Tensor& t, const char* name, long min_numel,
               const at::Tensor& like) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device() && t.is_contiguous() &&
                  t.scalar_type() == at::kLong && t.numel() >= min_numel,
              name, " must be a contiguous int64 tensor of at least ",
              min_numel, " elements on the logits' device");
}

template <typename T16, int G>
void launch_rows(int conf_mode, int grid, const at::Tensor& logits,
                 const long* ya, const long* yb, const float* lam, int B,
                 int C, int k, long long* slab, unsigned long long* conf) {
  pick<0, 1, 2>(conf_mode, [&](auto M) {
    const size_t lds = M == 1 ? (size_t)C * C * sizeof(int) : 0;
    launch256(meter_rows_kernel<T16, G, M>, dim3(grid), lds,
              (const T16*)logits.data_ptr(), ya, yb, lam, B, C, k, slab, conf);
  });
}

}  // namespace

// pack: lanes per row. 0 chooses (16 for C <= 16, else 64); 16 or 64 forces
// a layout (either runs any C: the lane loop covers the columns).
void meter_update(at::Tensor state, at::Tensor slab, at::Tensor logits,
                  at::Tensor y_a, c10::optional<at::Tensor> y_b,
                  c10::optional<at::Tensor> lam, long k,
                  c10::optional<at::Tensor> loss,
                  c10::optional<at::Tensor> confusion, long pack) {
  CHECK_GPU(logits);
  CHECK_CONTIG(logits);
  CHECK_16BIT(logits);
  TORCH_CHECK(logits.dim() == 2 && logits.size(0) >= 1 && logits.size(1) >= 1 &&
                  logits.size(0) <= INT_MAX && logits.size(1) <= INT_MAX,
              "logits must be (B,C) with B, C >= 1");
  const long B = logits.size(0), C = logits.size(1);
  TORCH_CHECK(k >= 1, "k must be at least 1, got ", k);
  TORCH_CHECK(y_b.has_value() == lam.has_value(),
              "y_b and lam come together (a mix target) or not at all");
  check_i64(state, "state", kMeterLen, logits);
  check_i64(slab, "slab", 4 * kMaxBlocks, logits);
  auto check_target = [&](const at::Tensor& t, const char* name) {
    check_i64(t, name, B, logits);
    TORCH_CHECK(t.dim() == 1 && t.size(0) == B, name, " must have shape (B,)");
  };
  check_target(y_a, "y_a");
  if (y_b) check_target(*y_b, "y_b");
  if (lam)
    TORCH_CHECK(lam->is_cuda() && lam->device() == logits.device() &&
                    lam->is_contiguous() && lam->scalar_type() == at::kFloat &&
                    lam->dim() == 1 && lam->size(0) == B,
                "lam must be a contiguous (B,) float32 tensor on the logits' "
                "device");
  const float* loss_ptr = nullptr;
  if (loss) {
    TORCH_CHECK(loss->is_cuda() && loss->device() == logits.device() &&
                    loss->scalar_type() == at::kFloat && loss->numel() == 1,
                "loss must be one float32 element on the logits' device");
    loss_ptr = loss->data_ptr<float>();
  }
  int conf_mode = 0;
  unsigned long long* conf_ptr = nullptr;
  if (confusion) {
    check_i64(*confusion, "confusion", C * C, logits);
    TORCH_CHECK(confusion->numel() == C * C, "confusion must be (C,C)");
    conf_mode = C <= kTileMaxC ? 1 : 2;
    conf_ptr = reinterpret_cast<unsigned long long*>(confusion->data_ptr<long>());
  }
  TORCH_CHECK(pack == 0 || pack == 16 || pack == 64,
              "pack must be 0, 16 or 64, got ", pack);
  const int G = pack ? (int)pack : (C <= 16 ? 16 : 64);
  const int grid =
      (int)std::max<long>(1, std::min<long>(cdiv_l(B, 256 / G), kMaxBlocks));
  const int kk = (int)std::min<long>(k, INT_MAX);
  long long* sl = reinterpret_cast<long long*>(slab.data_ptr<long>());
  const long* yb_ptr = y_b ? y_b->data_ptr<long>() : nullptr;
  const float* lam_ptr = lam ? lam->data_ptr<float>() : nullptr;
  DISPATCH_16(logits, T16, {
    pick<16, 64>(G, [&](auto GG) {
      launch_rows<T16, GG>(conf_mode, grid, logits, y_a.data_ptr<long>(),
                           yb_ptr, lam_ptr, (int)B, (int)C, kk, sl, conf_ptr);
    });
  });
  hipLaunchKernelGGL(meter_finalise_kernel, dim3(1), dim3(256), 0, cur_stream(),
                     sl, grid, (int)B, loss_ptr,
                     reinterpret_cast<long long*>(state.data_ptr<long>()));
}
