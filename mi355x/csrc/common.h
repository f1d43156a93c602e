// Shared helpers for the mi355x gfx950 kernel library.
// Native HIP for CDNA4 only — no CUDA dual path, no hipify.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#define DEV_INLINE __device__ __forceinline__

// 16-bit element traits: T16 is __hip_bfloat16 or __half.
template <typename T16>
struct F16 {};

template <>
struct F16<__hip_bfloat16> {
  static DEV_INLINE float to_f32(__hip_bfloat16 v) { return __bfloat162float(v); }
  static DEV_INLINE __hip_bfloat16 from_f32(float f) { return __float2bfloat16(f); }
};

template <>
struct F16<__half> {
  static DEV_INLINE float to_f32(__half v) { return __half2float(v); }
  static DEV_INLINE __half from_f32(float f) { return __float2half(f); }
};

// 8 x 16-bit lane vector (16 B — the CDNA4 coalescing sweet spot, guide G13).
typedef __attribute__((ext_vector_type(8))) short short8;
typedef __attribute__((ext_vector_type(4))) short short4v;
typedef __attribute__((ext_vector_type(4))) float float4v;
typedef __attribute__((ext_vector_type(4))) int int4v;

constexpr int kWave = 64;  // CDNA4 wavefront width

__host__ __device__ inline int cdiv_i(int a, int b) { return (a + b - 1) / b; }
static inline long cdiv_l(long a, long b) { return (a + b - 1) / b; }

// bit-exact short <-> 16-bit float element moves (vector lanes carry shorts)
template <typename T16>
DEV_INLINE float s16_to_f32(short v) {
  T16 t;
  __builtin_memcpy(&t, &v, 2);
  return F16<T16>::to_f32(t);
}

template <typename T16>
DEV_INLINE short f32_to_s16(float f) {
  T16 t = F16<T16>::from_f32(f);
  short v;
  __builtin_memcpy(&v, &t, 2);
  return v;
}

// ReLU of every fused epilogue. Equal to fmaxf(v, 0.f) for every number
// (-0 gives +0 too) but a NaN stays a NaN, as in torch.relu: fmaxf would
// return 0, and an overflow that became NaN in the forward pass would then
// train on as a clean zero where the loss scaler can never see it.
// IEEE-754-2019 maximum: one v_maximum3_f32 on gfx950 (fmaxf is two v_max).
DEV_INLINE float relu_f(float v) {
  return __builtin_elementwise_maximum(v, 0.f);
}

#define CHECK_GPU(x) TORCH_CHECK((x).is_cuda(), #x " must be on GPU")
#define CHECK_CONTIG(x) TORCH_CHECK((x).is_contiguous(), #x " must be contiguous")
#define CHECK_16BIT(x)                                       \
  TORCH_CHECK((x).scalar_type() == at::kBFloat16 ||          \
                  (x).scalar_type() == at::kHalf,            \
              #x " must be bf16 or fp16")

// Dispatch on the 16-bit activation dtype.
#define DISPATCH_16(TENSOR, T16, ...)                  \
  do {                                                 \
    if ((TENSOR).scalar_type() == at::kBFloat16) {     \
      using T16 = __hip_bfloat16;                      \
      __VA_ARGS__;                                     \
    } else {                                           \
      using T16 = __half;                              \
      __VA_ARGS__;                                     \
    }                                                  \
  } while (0)

static inline hipStream_t cur_stream() {
  return (hipStream_t)at::cuda::getCurrentCUDAStream().stream();
}

// Launch `kern` with 256 threads on the current stream. Each argument is
// converted to the kernel's parameter type, as in a plain call.
template <typename... P, typename... A>
static inline void launch256(void (*kern)(P...), dim3 grid, size_t lds_bytes,
                             A&&... args) {
  hipLaunchKernelGGL(kern, grid, dim3(256), lds_bytes, cur_stream(),
                     static_cast<P>(args)...);
}

// Runtime value -> template argument: calls f(std::integral_constant<.., V>)
// for the V in Vs that equals v, so a launcher names its kernel once and the
// listed values are exactly the variants that get instantiated.
//   pick<4, 2>(nt, [&](auto NT) { launch256(kern<T16, NT>, ...); });
template <auto... Vs, typename T, typename F>
static inline void pick(T v, F&& f) {
  const bool hit =
      ((v == Vs ? (f(std::integral_constant<decltype(Vs), Vs>{}), true)
                : false) || ...);
  TORCH_CHECK(hit, "pick: no kernel variant for this value");
}

// The library's environment knobs (MI355X_*, listed in the README) all go
// through this reader. Keep the result in a function-local static: a knob
// is read once per process, never per launch.
struct EnvKnob {
  const char* val;
  explicit EnvKnob(const char* name) : val(getenv(name)) {}
  // on/off knob that defaults to on: only a leading '0' turns it off
  bool on() const { return !val || val[0] != '0'; }
  long num(long dflt) const { return val ? atol(val) : dflt; }
};

// Split `total` items into about `want` chunks of equal size, a multiple of
// `granule`: {items per chunk, chunks actually needed}.
struct SplitPlan {
  long per, n;
};
static inline SplitPlan split_plan(long total, long want, long granule = 1) {
  const long per =
      cdiv_l(cdiv_l(total, std::max<long>(want, 1)), granule) * granule;
  return {per, cdiv_l(total, per)};
}

// out[e] = sum_z part[z][e], always added in the same order, so split
// reductions that store per-block partial rows and fold them here give
// bit-identical results from run to run (float atomicAdd onto the output
// does not: the order the blocks arrive in varies). A block covers 32
// elements x 32 interleaved z-slices (few dependent loads per thread: the
// fold is latency-bound); the slices meet in LDS.
static __global__ __launch_bounds__(1024) void fold_rows_kernel(
    const float* __restrict__ part, float* __restrict__ out, long E, int nz) {
  __shared__ float l[32][32];
  const int le = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const long e = (long)blockIdx.x * 32 + le;
  float a = 0.f;
  if (e < E) {
#pragma unroll 8
    for (int z = sl; z < nz; z += 32) a += part[(long)z * E + e];
  }
  l[sl][le] = a;
  __syncthreads();
  if (sl == 0 && e < E) {
    float s = l[0][le];
#pragma unroll
    for (int j = 1; j < 32; ++j) s += l[j][le];
    out[e] = s;
  }
}

// the same fold for a few rows (split-M wgrads of large filters: nz of
// 2..8 over up to millions of elements): one element per thread, every
// lane busy, rows added in order
static __global__ __launch_bounds__(256) void fold_few_rows_kernel(
    const float* __restrict__ part, float* __restrict__ out, long E, int nz) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  float a = part[e];
  for (int z = 1; z < nz; ++z) a += part[(long)z * E + e];
  out[e] = a;
}

static inline void fold_rows(const at::Tensor& part, at::Tensor& out, long E,
                             long nz) {
  if (nz <= 8) {
    hipLaunchKernelGGL(fold_few_rows_kernel, dim3((unsigned)cdiv_l(E, 256)),
                       dim3(256), 0, cur_stream(), part.data_ptr<float>(),
                       out.data_ptr<float>(), E, (int)nz);
    return;
  }
  hipLaunchKernelGGL(fold_rows_kernel, dim3((unsigned)cdiv_l(E, 32)),
                     dim3(1024), 0, cur_stream(), part.data_ptr<float>(),
                     out.data_ptr<float>(), E, (int)nz);
}
