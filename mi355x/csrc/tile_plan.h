// The tile plan over the flat fp32 buffers that lars.hip and adam.hip walk:
// its constants, the per-tile decode, the per-tensor combine of the per-tile
// sums and the host-side checks. The plan's layout is documented at the top
// of lars.hip.
#pragma once

#include "common.h"
#include "guard.h"
#include "reduce.h"

#include <climits>
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

// The per-tensor combine of two per-tile slabs, by one block of kFinThreads:
// wave v owns tensors v, v+16, ...; lane l adds the tensor's tiles l, l+64,
// ... in double, then a butterfly. Lane 0 hands the sums to done(s, tens[s],
// sum_a, sum_b). One fixed order whatever the grid that filled the slabs.
template <typename F>
DEV_INLINE void combine_tiles(const float* __restrict__ slab_a,
                              const float* __restrict__ slab_b, int T,
                              const int4v* __restrict__ tens, int S,
                              F&& done) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int s = wave; s < S; s += kFinWaves) {
    const int4v e = tens[s];
    const int t0 = max(e[0], 0), t1 = min(e[1], T);
    double a = 0.0, b = 0.0;
    for (int t = t0 + lane; t < t1; t += kWave) {
      a += (double)slab_a[t];
      b += (double)slab_b[t];
    }
    a = wave_sum(a);
    b = wave_sum(b);
    if (lane == 0) done(s, e, a, b);
  }
}

inline void check_i32x4(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == at::kInt, name, " must be int32");
  TORCH_CHECK(t.dim() == 2 && t.size(1) == 4, name, " must be [rows, 4]");
}

// the rows of a checked plan table as the kernels read them
inline const int4v* int4_rows(const at::Tensor& t) {
  return reinterpret_cast<const int4v*>(t.data_ptr<int>());
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

// what every plan entry point takes: p and g, the guard state and the plan
inline PlanDims check_plan(const at::Tensor& p, const at::Tensor& g,
                           const at::Tensor& state, const at::Tensor& table,
                           const at::Tensor& tens, const at::Tensor& stats) {
  const long n = p.numel();
  check_flat(p, "p", n);
  check_flat(g, "g", n);
  check_f32(state, "state", kStateLen);
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
