// The guard state shared by the guarded optimizer steps (gradstat.hip,
// lars.hip): its layout, the multiplier derived from it, and the non-finite
// test. Layout and rules are documented at the top of gradstat.hip.
#pragma once

#include "common.h"

#include <cmath>
#include <cstdint>

namespace {

enum GuardField {
  kScale = 0,
  kInvScale = 1,
  kTracker = 2,
  kSkipped = 3,
  kNonFinite = 4,
  kRawNorm = 5,
  kLastNorm = 6,
  kLastCoef = 7,
  kStateLen = 8,
};

// The step clock (layout and rules: gradstat.hip)
enum ClockField {
  kClkStep = 0,
  kClkLr = 1,
  kClkEmaOmd = 2,
  kClkLen = 4,
};

// e += omd * (w - e), w the weight just written. The roundings spelled out
// as in lars_elem, so every update kernel averages alike.
DEV_INLINE void ema_elem(float& e, float w, float omd) {
#pragma clang fp contract(off)
  e = fmaf(omd, w - e, e);
}

// inf or nan by the exponent field alone: a finite 3e38 stays finite here
// although its square overflows
DEV_INLINE int non_finite(float v) {
  return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u;
}

struct GuardCoef {
  float norm, coef, eff;
};

// norm of the true (unscaled, world-averaged) gradient, the clip coefficient
// and the multiplier the step applies. With no scaler (inv_scale == 1) and
// max_norm == +inf, eff == gscale exactly.
DEV_INLINE GuardCoef guard_coef_of(float raw_norm, float inv_scale,
                                   float gscale, float max_norm) {
  // every product rounded on its own: the step and the update kernel (and
  // the CPU fallback) then agree on all three values to the bit
#pragma clang fp contract(off)
  GuardCoef r;
  const float k = gscale * inv_scale;
  r.norm = raw_norm * k;
  r.coef = isinf(max_norm) ? 1.f : fminf(1.f, max_norm / (r.norm + 1e-6f));
  r.eff = k * r.coef;
  return r;
}

DEV_INLINE GuardCoef guard_coef(const float* st, float gscale,
                                float max_norm) {
  return guard_coef_of(st[kRawNorm], st[kInvScale], gscale, max_norm);
}

inline void check_f32(const at::Tensor& t, const char* name, long min_numel) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == at::kFloat, name, " must be float32");
  TORCH_CHECK(t.numel() >= min_numel, name, " needs at least ", min_numel,
              " elements");
}

// a learning rate read on the device: one float32 element next to p
inline const float* check_dev_scalar(const at::Tensor& lr, const at::Tensor& p) {
  check_f32(lr, "lr", 1);
  TORCH_CHECK(lr.numel() == 1, "a tensor lr must hold one element");
  TORCH_CHECK(lr.device() == p.device(),
              "a tensor lr must live on the buffers' device");
  return lr.data_ptr<float>();
}

struct EmaArgs {
  float* e;
  const float* clock;
};

// the EMA buffer (p's size, 16-byte aligned like it) and the clock it needs
inline EmaArgs check_ema(const at::Tensor& ema,
                         const c10::optional<at::Tensor>& clock,
                         const at::Tensor& p) {
  check_f32(ema, "ema", 0);
  TORCH_CHECK(ema.numel() == p.numel(), "ema must have ", p.numel(),
              " elements like the parameters");
  TORCH_CHECK(ema.device() == p.device(),
              "ema must live on the parameters' device");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(ema.data_ptr<float>()) % 16 == 0,
              "ema must start at a 16-byte aligned address");
  TORCH_CHECK(clock.has_value(), "an EMA update needs the step clock");
  check_f32(*clock, "clock", kClkLen);
  TORCH_CHECK(clock->device() == p.device(),
              "the clock must live on the parameters' device");
  return {ema.data_ptr<float>(), clock->data_ptr<float>()};
}

}  // namespace
