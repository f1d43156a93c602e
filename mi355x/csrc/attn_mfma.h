// The small MFMA helpers shared by the two attention files: attn.hip (a whole
// head resident, S <= 256) and attn_flash.hip (keys streamed, S <= 4096).
// Both include it after their no-packed-fp32 and fp-contract pragmas, so that
// the helpers carry the attributes of the kernels they are inlined into.
#pragma once

#include "common.h"

typedef __attribute__((ext_vector_type(8))) _Float16 half8_a;
typedef __attribute__((ext_vector_type(16))) float f32x16_a;

namespace {

constexpr float kLog2e = 1.4426950408889634f;

// R x R output tile of one MFMA: A lane l holds row l % R, k-slots
// (l / R) * 8 + e; B the same with columns; D lane l holds column l % R and,
// in register r, row (r & 3) + 8 * (r >> 2) + 4 * (l / R).
template <typename T16, int R>
struct AMfma;
template <>
struct AMfma<__hip_bfloat16, 32> {
  typedef f32x16_a acc;
  static DEV_INLINE acc run(short8 a, short8 b, acc c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
};
template <>
struct AMfma<__half, 32> {
  typedef f32x16_a acc;
  static DEV_INLINE acc run(short8 a, short8 b, acc c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16((half8_a)a, (half8_a)b, c, 0,
                                                  0, 0);
  }
};
template <>
struct AMfma<__hip_bfloat16, 16> {
  typedef float4v acc;
  static DEV_INLINE acc run(short8 a, short8 b, acc c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
};
template <>
struct AMfma<__half, 16> {
  typedef float4v acc;
  static DEV_INLINE acc run(short8 a, short8 b, acc c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16((half8_a)a, (half8_a)b, c, 0,
                                                  0, 0);
  }
};

DEV_INLINE int acc_row(int r, int kg) { return (r & 3) + 8 * (r >> 2) + 4 * kg; }

DEV_INLINE short8 ld16(const short* p) {
  return *reinterpret_cast<const short8*>(p);
}

DEV_INLINE short8 cat4(const short* p0, const short* p1) {
  const short4v a = *reinterpret_cast<const short4v*>(p0);
  const short4v b = *reinterpret_cast<const short4v*>(p1);
  return short8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

}  // namespace
