// The fixed-order sums of the optimizer kernels (gradstat.hip, lars.hip,
// adam.hip): a wave butterfly and the 256-thread block sum. Every norm, count
// and trust ratio goes through these, so its bits do not depend on the grid.
#pragma once

#include "common.h"

namespace {

// xor butterfly from 32 down to 1: the sum, in every lane
template <typename T>
DEV_INLINE T wave_sum(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

// four partial sums in the one order every sum here uses: the lane
// accumulators of a 16 B/lane sweep, and the four wave slots of a block
template <typename T>
DEV_INLINE T sum4(T a0, T a1, T a2, T a3) {
  return (a0 + a1) + (a2 + a3);
}

// Sums each of v... over a block of 256 threads: a wave butterfly, one LDS
// slot per wave, then thread 0 adds the slots with sum4. Only thread 0 holds
// the sums afterwards. float, int, double or long long, in any mix; the
// butterflies of all values advance together, so they overlap. Every thread
// of the block calls it. A kernel that calls it again (a loop over tiles)
// puts a __syncthreads() in between: the slots are reused.
template <typename... T>
DEV_INLINE void block_sum256(T&... v) {
  static_assert(((sizeof(T) <= 8) && ...), "a slot holds 8 bytes");
  __shared__ double rows[sizeof...(T)][4];  // raw: row i is four slots of T_i
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    ((v += __shfl_xor(v, off, kWave)), ...);
  void* row = rows;
  if ((threadIdx.x & 63) == 0)
    ((static_cast<T*>(row)[threadIdx.x >> 6] = v, row = (double*)row + 4), ...);
  __syncthreads();
  if (threadIdx.x == 0) {
    row = rows;
    ((v = sum4(static_cast<T*>(row)[0], static_cast<T*>(row)[1],
               static_cast<T*>(row)[2], static_cast<T*>(row)[3]),
      row = (double*)row + 4),
     ...);
  }
}

}  // namespace
