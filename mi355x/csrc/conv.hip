// NHWC conv2d: forward, dgrad, wgrad (SURVEY.md N5 — the reference's
// cuDNN/MIOpen implicit-GEMM conv, rebuilt for CDNA4).
//
// Three tiers live here:
//  - direct kernels (correctness-first fallback for odd geometries and the
//    on-device numerics reference), C channel-minor coalesced everywhere;
//  - small-C register-window kernels (C=3/6 stems the MFMA path cannot
//    tile: C % 64 != 0);
//  - LDS-staged stem kernels (7x7/s2 ImageNet and 3x3/s1 CIFAR stems):
//    one block stages the input strip for an output row cooperatively,
//    taps are LDS reads, packed bf16 v_dot2c (7x7) or plain f32 FMA (3x3)
//    accumulation. These replaced the register-window variants for those
//    shapes after PMC showed them latency-bound (profiles/).
// The MFMA implicit-GEMM path (conv_mfma.hip) takes every C%64==0 shape.
#include "conv_internal.h"

namespace {

template <typename T16>
__global__ void conv_fwd_direct(const T16* __restrict__ x,
                                const T16* __restrict__ w,
                                const float* __restrict__ bias,
                                T16* __restrict__ y, int N, int H, int W,
                                int C, int K, int R, int S, int P, int Q,
                                int stride, int pad, int act, int has_bias) {
  const long total = (long)N * P * Q * K;
  const bool cvec = (C % 8 == 0);
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (long)gridDim.x * blockDim.x) {
    const int k = (int)(t % K);
    long npq = t / K;
    const int q = (int)(npq % Q);
    long np = npq / Q;
    const int p = (int)(np % P);
    const int n = (int)(np / P);
    float acc = has_bias ? bias[k] : 0.f;
    const T16* wk = w + (long)k * R * S * C;
    for (int r = 0; r < R; ++r) {
      const int ih = p * stride - pad + r;
      if (ih < 0 || ih >= H) continue;
      for (int s = 0; s < S; ++s) {
        const int iw = q * stride - pad + s;
        if (iw < 0 || iw >= W) continue;
        const T16* xp = x + (((long)n * H + ih) * W + iw) * C;
        const T16* wp = wk + (long)(r * S + s) * C;
        if (cvec) {
          for (int c = 0; c < C; c += 8) {
            short8 xv = *reinterpret_cast<const short8*>(xp + c);
            short8 wv = *reinterpret_cast<const short8*>(wp + c);
#pragma unroll
            for (int u = 0; u < 8; ++u)
              acc += s16_to_f32<T16>(xv[u]) * s16_to_f32<T16>(wv[u]);
          }
        } else {
          for (int c = 0; c < C; ++c)
            acc += F16<T16>::to_f32(xp[c]) * F16<T16>::to_f32(wp[c]);
        }
      }
    }
    if (act == 1) acc = relu_f(acc);
    y[t] = F16<T16>::from_f32(acc);
  }
}

// weights in the transposed [R,S,C,K] layout (wt[r,s,c,k] = w[k,c,r,s]):
// the k-loop reads are contiguous per lane (vectorized when K % 8 == 0)
template <typename T16>
__global__ void conv_dgrad_direct(const T16* __restrict__ dy,
                                  const T16* __restrict__ wt,
                                  T16* __restrict__ dx, int N, int H, int W,
                                  int C, int K, int R, int S, int P, int Q,
                                  int stride, int pad) {
  const long total = (long)N * H * W * C;
  const bool kvec = (K % 8 == 0);
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (long)gridDim.x * blockDim.x) {
    const int c = (int)(t % C);
    long nhw = t / C;
    const int iw = (int)(nhw % W);
    long nh = nhw / W;
    const int ih = (int)(nh % H);
    const int n = (int)(nh / H);
    float acc = 0.f;
    for (int r = 0; r < R; ++r) {
      const int ph = ih + pad - r;
      if (ph < 0 || ph % stride) continue;
      const int p = ph / stride;
      if (p >= P) continue;
      for (int s = 0; s < S; ++s) {
        const int qw = iw + pad - s;
        if (qw < 0 || qw % stride) continue;
        const int q = qw / stride;
        if (q >= Q) continue;
        const T16* dyp = dy + (((long)n * P + p) * Q + q) * K;
        const T16* wp = wt + ((long)(r * S + s) * C + c) * K;
        if (kvec) {
          for (int k = 0; k < K; k += 8) {
            short8 dv = *reinterpret_cast<const short8*>(dyp + k);
            short8 wv = *reinterpret_cast<const short8*>(wp + k);
#pragma unroll
            for (int u = 0; u < 8; ++u)
              acc += s16_to_f32<T16>(dv[u]) * s16_to_f32<T16>(wv[u]);
          }
        } else {
          for (int k = 0; k < K; ++k)
            acc += F16<T16>::to_f32(dyp[k]) * F16<T16>::to_f32(wp[k]);
        }
      }
    }
    dx[t] = F16<T16>::from_f32(acc);
  }
}

template <typename T16>
__global__ void conv_wgrad_direct(const T16* __restrict__ x,
                                  const T16* __restrict__ dy,
                                  float* __restrict__ dw, int N, int H, int W,
                                  int C, int K, int R, int S, int P, int Q,
                                  int stride, int pad, long m_per_chunk) {
  const long total_w = (long)K * R * S * C;
  const long M = (long)N * P * Q;
  const long m0 = (long)blockIdx.y * m_per_chunk;
  const long m1 = min(M, m0 + m_per_chunk);
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total_w;
       t += (long)gridDim.x * blockDim.x) {
    const int c = (int)(t % C);
    const int s = (int)((t / C) % S);
    const int r = (int)((t / ((long)C * S)) % R);
    const int k = (int)(t / ((long)C * S * R));
    float acc = 0.f;
    // incremental (n,p,q) decode: one div/mod at entry, carries after
    int q = (int)(m0 % Q);
    long np0 = m0 / Q;
    int p = (int)(np0 % P);
    int n = (int)(np0 / P);
    for (long m = m0; m < m1; ++m) {
      const int ih = p * stride - pad + r;
      const int iw = q * stride - pad + s;
      if (ih >= 0 && ih < H && iw >= 0 && iw < W)
        acc += F16<T16>::to_f32(dy[m * K + k]) *
               F16<T16>::to_f32(x[(((long)n * H + ih) * W + iw) * C + c]);
      if (++q == Q) {
        q = 0;
        if (++p == P) {
          p = 0;
          ++n;
        }
      }
    }
    // store in the parameter layout [K,C,R,S]
    // (split-M: one partial filter per chunk, folded in order by fold_rows)
    dw[(long)blockIdx.y * total_w + ((long)k * C + c) * ((long)R * S) +
       (long)r * S + s] = acc;
  }
}

inline dim3 conv_grid(long total, int block = 256, int cap = 4096) {
  return dim3((unsigned)std::min<long>(cdiv_l(total, block), cap));
}

// ---- small-C fwd (stems: 3x3, C=3/6, K<=64, stride 1/2) ----------------
// lane = output channel k; the 3x3xC input window and the lane's weights
// live in REGISTERS; x loads are wave-uniform (one k-row broadcast) and
// the window slides along q so each output costs R*stride*C new loads.
template <typename T16, int C_, int S_>
__global__ __launch_bounds__(256) void conv_fwd_smallc(
    const T16* __restrict__ x, const T16* __restrict__ wgt,
    const float* __restrict__ bias, const T16* __restrict__ zpage,
    T16* __restrict__ y, int N, int H, int W,
    int K, int Ho, int Wo, int stride, int pad, long wrow_stride, int act,
    int has_bias, long m_per_chunk, long Mtot) {
  const int k = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  // per-lane weights: w[r][s][c] from [K][kg] (kg=(r*S+s)*C+c, maybe padded)
  float wr[S_ * S_ * C_];
  {
    const T16* wp = wgt + (long)min(k, K - 1) * wrow_stride;
#pragma unroll
    for (int i = 0; i < S_ * S_ * C_; ++i) wr[i] = F16<T16>::to_f32(wp[i]);
  }
  const float bk = has_bias ? bias[min(k, K - 1)] : 0.f;

  const long m_begin = (long)blockIdx.x * m_per_chunk;
  const long m_end = min(Mtot, m_begin + m_per_chunk);
  const long per_wave = (m_end - m_begin + 3) / 4;
  long w0 = m_begin + wv * per_wave;
  const long w1 = min(m_end, w0 + per_wave);
  if (w0 >= w1) return;

  int q = (int)(w0 % Wo);
  long np = w0 / Wo;
  int p = (int)(np % Ho);
  int n = (int)(np / Ho);

  float xw[S_ * S_ * C_];  // sliding window [r][s][c]
  bool fresh = true;
  for (long m = w0; m < w1; ++m) {
    const int ih0 = p * stride - pad;
    const int iw0 = q * stride - pad;
    if (fresh) {
#pragma unroll
      for (int r = 0; r < S_; ++r) {
        const int ih = ih0 + r;
        const bool rok = (unsigned)ih < (unsigned)H;
        const T16* row = rok ? x + ((long)n * H + ih) * W * C_ : zpage;
#pragma unroll
        for (int ss = 0; ss < S_; ++ss) {
          const int iw = iw0 + ss;
          const bool ok = rok && (unsigned)iw < (unsigned)W;
          // address-select (zero page), never a branch around the load:
          // per-element branchy loads serialize one vmcnt wait each
          const T16* src = ok ? row + (long)iw * C_ : zpage;
#pragma unroll
          for (int c = 0; c < C_; ++c)
            xw[(r * S_ + ss) * C_ + c] = F16<T16>::to_f32(src[c]);
        }
      }
      fresh = false;
    } else {
      // slide: shift left by `stride` columns, load the new ones
      if (stride == 1) {
#pragma unroll
        for (int r = 0; r < S_; ++r)
#pragma unroll
          for (int ss = 0; ss < S_ - 1; ++ss)
#pragma unroll
            for (int c = 0; c < C_; ++c)
              xw[(r * S_ + ss) * C_ + c] = xw[(r * S_ + ss + 1) * C_ + c];
      } else {
#pragma unroll
        for (int r = 0; r < S_; ++r)
#pragma unroll
          for (int ss = 0; ss < S_ - 2; ++ss)
#pragma unroll
            for (int c = 0; c < C_; ++c)
              xw[(r * S_ + ss) * C_ + c] = xw[(r * S_ + ss + 2) * C_ + c];
      }
      // new right-hand columns: compile-time ss indices (a runtime index
      // into xw[] would force the whole window to scratch — rule 20)
#pragma unroll
      for (int r = 0; r < S_; ++r) {
        const int ih = ih0 + r;
        const bool rok = (unsigned)ih < (unsigned)H;
        const T16* row = rok ? x + ((long)n * H + ih) * W * C_ : zpage;
        if (stride == 1) {
          constexpr int ss = S_ - 1;
          const int iw = iw0 + ss;
          const bool ok = rok && (unsigned)iw < (unsigned)W;
          const T16* src = ok ? row + (long)iw * C_ : zpage;
#pragma unroll
          for (int c = 0; c < C_; ++c)
            xw[(r * S_ + ss) * C_ + c] = F16<T16>::to_f32(src[c]);
        } else {
#pragma unroll
          for (int jj = 0; jj < 2; ++jj) {
            const int ss = S_ - 2 + jj;
            const int iw = iw0 + ss;
            const bool ok = rok && (unsigned)iw < (unsigned)W;
            const T16* src = ok ? row + (long)iw * C_ : zpage;
#pragma unroll
            for (int c = 0; c < C_; ++c)
              xw[(r * S_ + ss) * C_ + c] = F16<T16>::to_f32(src[c]);
          }
        }
      }
    }
    float acc = bk;
#pragma unroll
    for (int i = 0; i < S_ * S_ * C_; ++i) acc += xw[i] * wr[i];
    if (act == 1) acc = relu_f(acc);
    if (k < K) y[m * K + k] = F16<T16>::from_f32(acc);
    if (++q == Wo) {
      q = 0;
      fresh = true;
      if (++p == Ho) {
        p = 0;
        ++n;
      }
    }
  }
}

// ---- packed bf16/f16 dot2 helpers (stem kernels) -----------------------
template <typename T16>
struct Dot2;
template <>
struct Dot2<__hip_bfloat16> {
  typedef __bf16 v2 __attribute__((ext_vector_type(2)));
  static __device__ __forceinline__ float fma(v2 a, v2 b, float c) {
    return __builtin_amdgcn_fdot2_f32_bf16(a, b, c, false);
  }
};
template <>
struct Dot2<__half> {
  typedef _Float16 v2 __attribute__((ext_vector_type(2)));
  static __device__ __forceinline__ float fma(v2 a, v2 b, float c) {
    return __builtin_amdgcn_fdot2(a, b, c, false);
  }
};

template <typename T16>
__device__ __forceinline__ typename Dot2<T16>::v2 pack2(T16 a, T16 b) {
  unsigned u;
  unsigned short lo, hi;
  __builtin_memcpy(&lo, &a, 2);
  __builtin_memcpy(&hi, &b, 2);
  u = (unsigned)lo | ((unsigned)hi << 16);
  typename Dot2<T16>::v2 r;
  __builtin_memcpy(&r, &u, 4);
  return r;
}

// ---- LDS strip shared by the stem kernels and their launchers -----------
// A strip holds the input rows under one output row: `rows` rows of
// `selems` elements. +4: 8B-aligned row stride with >=1 zeroed pad element
// (the 7x7 fwd's pair 10 reads element 6q+21, one past the last tap).
struct StripGeom {
  int sstride;  // row stride, elements
  int bytes;    // whole strip
};
__host__ __device__ inline StripGeom strip_geom(int rows, int selems,
                                                int elem_bytes) {
  const int sstride = (selems + 4) & ~3;
  return {sstride, rows * sstride * elem_bytes};
}
__host__ __device__ inline StripGeom stem7_strip(int Wo, int elem_bytes) {
  return strip_geom(7, (2 * Wo + 5) * 3, elem_bytes);
}
__host__ __device__ inline StripGeom stem3_strip(int Wo) {
  return strip_geom(3, (Wo + 2) * 3, 4);
}

template <typename D, typename T16>
DEV_INLINE D strip_cvt(T16 v) {
  if constexpr (std::is_same<D, float>::value)
    return F16<T16>::to_f32(v);
  else
    return v;
}

// Cooperative strip fill (256 threads): rows ih0 .. ih0+ROWS-1 of image n,
// kept as D = T16 or converted once to D = float. Strip element
// (iw+pad)*3+c maps to the CONTIGUOUS x row element iw*3+c, so the
// interior is short8 block copies (the elementwise /3-decode version was
// ~19 serial 2B loads per thread); pads and invalid rows are zeroed.
// off3 = 3*pad strip elements precede the payload. With D = T16 the short8
// store lands on a 2-byte-aligned LDS address when off3 is odd: only the
// 7x7 fwd stem uses that form.
template <int ROWS, typename D, typename T16>
DEV_INLINE void strip_fill(D* xs, const T16* x, int n, int H, int W, int ih0,
                           int off3, int sstride) {
  const D z{};
  const int row3 = 3 * W;  // contiguous payload per row
  const int nv8 = (row3 + 7) / 8;
  for (int t = threadIdx.x; t < ROWS * nv8; t += 256) {
    const int rr = t / nv8;
    const int j8 = (t - rr * nv8) * 8;
    const int ih = ih0 + rr;
    D* dst = xs + (long)rr * sstride + off3 + j8;
    if ((row3 & 7) == 0 && (unsigned)ih < (unsigned)H && j8 + 8 <= row3) {
      const short8 v = *reinterpret_cast<const short8*>(
          x + ((long)n * H + ih) * row3 + j8);
      if constexpr (std::is_same<D, float>::value) {
#pragma unroll
        for (int u = 0; u < 8; ++u) dst[u] = s16_to_f32<T16>(v[u]);
      } else {
        *reinterpret_cast<short8*>(dst) = v;
      }
    } else {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = j8 + u;
        dst[u] = (e < row3 && (unsigned)ih < (unsigned)H)
                     ? strip_cvt<D>(x[((long)n * H + ih) * row3 + e])
                     : z;
      }
    }
  }
  // zero the pad columns (and the alignment tail) of every row
  for (int t = threadIdx.x; t < ROWS * (sstride - row3); t += 256) {
    const int nz = sstride - row3;
    const int rr = t / nz;
    const int e = t - rr * nz;
    xs[(long)rr * sstride + (e < off3 ? e : row3 + e)] = z;
  }
}

// one dy output row (n elements, coalesced) into LDS for the stem wgrads
template <typename T16>
DEV_INLINE void stage_dy_row(T16* dys, const T16* dyrow, int n) {
  if ((n & 7) == 0) {
    for (int i = threadIdx.x * 8; i < n; i += 256 * 8)
      *reinterpret_cast<short8*>(dys + i) =
          *reinterpret_cast<const short8*>(dyrow + i);
  } else {
    for (int i = threadIdx.x; i < n; i += 256) dys[i] = dyrow[i];
  }
}

// ---- 7x7/stride-2 stem fwd v3: cooperative LDS staging -----------------
// v2 (register sliding window) measured latency-bound: each wave had ~1
// cache line in flight, issued right before use. v3 stages the whole
// 7-row input strip for one output row COOPERATIVELY (256 threads, fully
// coalesced, many lines in flight), then the inner loop reads taps from
// LDS only: per output 77 ds_read_b32 (wave-uniform broadcast, 4B-aligned
// since the pair stream starts at byte 12*q) + 77 v_dot2c. Weights stay in
// VGPRs (77 pairs); no circular buffer, no register shifting.
template <typename T16>
__global__ __launch_bounds__(256) void conv_fwd_stem7_lds(
    const T16* __restrict__ x, const T16* __restrict__ wgt,
    const float* __restrict__ bias, T16* __restrict__ y, int N, int H,
    int W, int K, int Ho, int Wo, int pad, long wrow_stride, int act,
    int has_bias) {
  using V2 = typename Dot2<T16>::v2;
  constexpr int ROWS = 7, WPAIR = 11;
  extern __shared__ char smem[];
  T16* xs = reinterpret_cast<T16*>(smem);
  const int sstride = stem7_strip(Wo, sizeof(T16)).sstride;

  const int p = blockIdx.x % Ho;
  const int n = blockIdx.x / Ho;
  const T16 z{};
  strip_fill<ROWS>(xs, x, n, H, W, 2 * p - pad, 3 * pad, sstride);

  const int k = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

  // per-lane packed weights (77 VGPR pairs)
  V2 wp[ROWS][WPAIR];
  {
    const T16* wk = wgt + (long)min(k, K - 1) * wrow_stride;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      const T16* wr = wk + r * 21;
#pragma unroll
      for (int u = 0; u < WPAIR - 1; ++u)
        wp[r][u] = pack2(wr[2 * u], wr[2 * u + 1]);
      wp[r][WPAIR - 1] = pack2(wr[20], z);
    }
  }
  const float bk = has_bias ? bias[min(k, K - 1)] : 0.f;
  __syncthreads();

  const int qper = (Wo + 3) / 4;
  const int q0 = wv * qper, q1 = min(Wo, q0 + qper);
  const long mrow = ((long)n * Ho + p) * Wo;
  for (int q = q0; q < q1; ++q) {
    float acc = bk;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      const V2* row = reinterpret_cast<const V2*>(
          reinterpret_cast<const char*>(xs + r * sstride) + 12 * q);
#pragma unroll
      for (int u = 0; u < WPAIR; ++u)
        acc = Dot2<T16>::fma(row[u], wp[r][u], acc);
    }
    if (act == 1) acc = relu_f(acc);
    if (k < K) y[(mrow + q) * K + k] = F16<T16>::from_f32(acc);
  }
}

// ---- 3x3/stride-1 CIFAR stem, LDS-staged (C=3, K<=64) ------------------
// Same strategy as the 7x7 stem: the register-window kernels were
// latency-bound on per-output wave-uniform loads (conv_fwd_smallc 224 us,
// conv_wgrad_smallc 301 us per call at b1024). One block stages the
// 3-row input strip for one output row as f32 (converted once), then
// taps are plain 4B-aligned LDS reads: fwd lane-per-k with 27 register
// weights; wgrad q-split waves with a 27-element f32 accumulator.
template <typename T16>
__global__ __launch_bounds__(256) void conv_fwd_stem3_lds(
    const T16* __restrict__ x, const T16* __restrict__ wgt,
    const float* __restrict__ bias, T16* __restrict__ y, int N, int H,
    int W, int K, int Ho, int Wo, long wrow_stride, int act, int has_bias) {
  extern __shared__ __attribute__((aligned(16))) char smem3[];
  float* xs = reinterpret_cast<float*>(smem3);
  const int sstride = stem3_strip(Wo).sstride;

  const int p = blockIdx.x % Ho;
  const int n = blockIdx.x / Ho;
  strip_fill<3>(xs, x, n, H, W, p - 1, 3, sstride);

  const int k = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float wr[27];
  {
    const T16* wk = wgt + (long)min(k, K - 1) * wrow_stride;
#pragma unroll
    for (int i = 0; i < 27; ++i) wr[i] = F16<T16>::to_f32(wk[i]);
  }
  const float bk = has_bias ? bias[min(k, K - 1)] : 0.f;
  __syncthreads();

  const int qper = (Wo + 3) / 4;
  const int q0 = wv * qper, q1 = min(Wo, q0 + qper);
  const long mrow = ((long)n * Ho + p) * Wo;
  for (int q = q0; q < q1; ++q) {
    float acc = bk;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const float* row = xs + r * sstride + 3 * q;
#pragma unroll
      for (int i = 0; i < 9; ++i) acc += row[i] * wr[r * 9 + i];
    }
    if (act == 1) acc = relu_f(acc);
    if (k < K) y[(mrow + q) * K + k] = F16<T16>::from_f32(acc);
  }
}

template <typename T16>
__global__ __launch_bounds__(256) void conv_wgrad_stem3_lds(
    const T16* __restrict__ x, const T16* __restrict__ dy,
    float* __restrict__ part,  // [gridDim.x*4][K*3*3*3]
    int N, int H, int W, int K, int Ho, int Wo, int rows_per_chunk) {
  extern __shared__ __attribute__((aligned(16))) char smem3[];
  const StripGeom sg = stem3_strip(Wo);
  const int sstride = sg.sstride;
  float* xs = reinterpret_cast<float*>(smem3);
  T16* dys = reinterpret_cast<T16*>(smem3 + sg.bytes);

  const int k = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long nrows = (long)N * Ho;
  const long row0 = (long)blockIdx.x * rows_per_chunk;
  const long row1 = min(nrows, row0 + rows_per_chunk);

  float acc[3][9] = {};
  const int qper = (Wo + 3) / 4;
  const int q0 = wv * qper, q1 = min(Wo, q0 + qper);

  for (long row = row0; row < row1; ++row) {
    const int p = (int)(row % Ho);
    const int n = (int)(row / Ho);
    __syncthreads();
    strip_fill<3>(xs, x, n, H, W, p - 1, 3, sstride);
    stage_dy_row(dys, dy + row * Wo * K, Wo * K);
    __syncthreads();

    for (int q = q0; q < q1; ++q) {
      const float dyv = (k < K) ? F16<T16>::to_f32(dys[q * K + k]) : 0.f;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const float* row_ = xs + r * sstride + 3 * q;
#pragma unroll
        for (int i = 0; i < 9; ++i) acc[r][i] += dyv * row_[i];
      }
    }
  }

  if (k < K) {
    const long E = (long)K * 27;
    float* slab = part + ((long)blockIdx.x * 4 + wv) * E;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        const int s = i / 3, c = i % 3;
        // parameter layout [K, C, R, S]
        slab[(((long)k * 3 + c) * 3 + r) * 3 + s] = acc[r][i];
      }
  }
}

// ---- 7x7/stride-2 stem wgrad (C=3, K<=64) ------------------------------
// Lane = output channel k; block (chunk, r) accumulates filter row r.
// dw[k, r, s, c] += dy[m, k] * x[m, tap(r,s,c)] over the block's m-range.
// The x tap row rides in a circular buffer of 18 f32 PAIRS (6-phase
// compile-time rotation, fresh columns loaded TWO outputs ahead so the
// load->fma dependency spans ~2 outputs of issue); the 21-tap accumulator
// is 11 packed pairs -> v_pk_fma_f32 (2 MACs/cycle). Replaces
// conv_wgrad_smallc for this shape (measured 5.8 ms/call on the ResNet-50
// stem: per-output serialized loads + scalar FMAs).
typedef float float2v __attribute__((ext_vector_type(2)));

// v3: cooperative LDS staging (same diagnosis as the fwd — v2 was
// latency-bound on the per-output dy line). A block walks a CHUNK of
// output rows; per row it stages the full 7-row-tall input strip is not
// needed — all 7 taps' source rows are staged as ONE f32 strip each? No:
// a single (n,p) output row reads input rows ih0..ih0+6; we stage all 7
// as f32 pairs (cvt paid once at staging) plus the dy row (bf16,
// coalesced), then each wave accumulates its q-subrange for ALL 7 filter
// rows: per output 1 dy ds_read + 7*11 ds_read_b64 (f32 pairs, 8B-aligned
// at byte 24q) + 7*11 v_pk_fma_f32. dy is read from HBM ONCE (the r-split
// variant re-read it 7x, latency-bound).
template <typename T16>
__global__ __launch_bounds__(256) void conv_wgrad_stem7_lds(
    const T16* __restrict__ x, const T16* __restrict__ dy,
    float* __restrict__ part,  // [gridDim.x*4][K*7*7*3]
    int N, int H, int W, int K, int Ho, int Wo, int pad, int rows_per_chunk) {
  constexpr int ROWS = 7, APAIR = 11;
  extern __shared__ char smem[];
  const StripGeom sg = stem7_strip(Wo, 4);      // f32 elems
  const int sstride = sg.sstride;
  float* xs = reinterpret_cast<float*>(smem);
  T16* dys = reinterpret_cast<T16*>(smem + sg.bytes);

  const int k = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long nrows = (long)N * Ho;
  const long row0 = (long)blockIdx.x * rows_per_chunk;
  const long row1 = min(nrows, row0 + rows_per_chunk);

  float2v acc[ROWS][APAIR] = {};

  const int qper = (Wo + 3) / 4;
  const int q0 = wv * qper, q1 = min(Wo, q0 + qper);

  for (long row = row0; row < row1; ++row) {
    const int p = (int)(row % Ho);
    const int n = (int)(row / Ho);
    __syncthreads();  // previous row's reads done before overwrite
    strip_fill<ROWS>(xs, x, n, H, W, 2 * p - pad, 3 * pad, sstride);
    stage_dy_row(dys, dy + row * Wo * K, Wo * K);
    __syncthreads();

    for (int q = q0; q < q1; ++q) {
      const float dyv = (k < K) ? F16<T16>::to_f32(dys[q * K + k]) : 0.f;
      float2v d2;
      d2.x = dyv;
      d2.y = dyv;
#pragma unroll
      for (int r = 0; r < ROWS; ++r) {
        const float2v* xrow = reinterpret_cast<const float2v*>(
            reinterpret_cast<const char*>(xs + r * sstride) + 24 * q);
#pragma unroll
        for (int u = 0; u < APAIR; ++u) acc[r][u] += d2 * xrow[u];
      }
    }
  }

  if (k < K) {
    const long E = (long)K * 7 * 7 * 3;
    float* slab = part + ((long)blockIdx.x * 4 + wv) * E;
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
      for (int u = 0; u < APAIR; ++u) {
        const int e0 = 2 * u, e1 = 2 * u + 1;
        const int s0 = e0 / 3, c0 = e0 % 3;
        slab[(((long)k * 3 + c0) * 7 + r) * 7 + s0] = acc[r][u].x;
        if (e1 < 21) {
          const int s1 = e1 / 3, c1 = e1 % 3;
          slab[(((long)k * 3 + c1) * 7 + r) * 7 + s1] = acc[r][u].y;
        }
      }
  }
}

// ---- small-C wgrad (stems: C=3/6, K<=64) -------------------------------
// lane = output channel k, all S_*C_ taps of one filter row r in REGISTERS
// (compile-time C_/S_ keep the accumulator array in VGPRs — guide rule
// 20); dy reads coalesced across lanes; x reads wave-uniform (broadcast).
// Each wave writes its own partial slab (no atomics); wgrad_reduce sums.
template <typename T16, int C_, int S_>
__global__ __launch_bounds__(256) void conv_wgrad_smallc(
    const T16* __restrict__ x, const T16* __restrict__ dy,
    const T16* __restrict__ zpage,
    float* __restrict__ part,  // [gridDim.x*4][K*R*S*C]
    int N, int H, int W, int K, int Ho, int Wo, int R, int stride, int pad,
    long m_per_chunk, long Mtot) {
  const int r = blockIdx.y;
  const int k = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  float acc[C_ * S_] = {};
  const long m_begin = (long)blockIdx.x * m_per_chunk;
  const long m_end = min(Mtot, m_begin + m_per_chunk);
  const long per_wave = (m_end - m_begin + 3) / 4;
  const long w0 = m_begin + wv * per_wave;
  const long w1 = min(m_end, w0 + per_wave);
  if (w0 < w1) {
    int q = (int)(w0 % Wo);
    long np = w0 / Wo;
    int p = (int)(np % Ho);
    int n = (int)(np / Ho);
    // sliding x window for the fixed filter row r: S_*C_ values, shifted
    // by `stride` columns per output step (wave-uniform loads)
    float xq[S_ * C_];
    bool fresh = true;
    for (long m = w0; m < w1; ++m) {
      const int ih = p * stride - pad + r;
      const bool rok = (unsigned)ih < (unsigned)H;
      const T16* row = rok ? x + ((long)n * H + ih) * W * C_ : zpage;
      const int iw0 = q * stride - pad;
      if (fresh || !rok) {
#pragma unroll
        for (int s = 0; s < S_; ++s) {
          const int iw = iw0 + s;
          const bool ok = rok && (unsigned)iw < (unsigned)W;
          const T16* src = ok ? row + (long)iw * C_ : zpage;
#pragma unroll
          for (int c = 0; c < C_; ++c)
            xq[s * C_ + c] = F16<T16>::to_f32(src[c]);
        }
        fresh = false;
      } else {
        if (stride == 1) {
#pragma unroll
          for (int i = 0; i < (S_ - 1) * C_; ++i) xq[i] = xq[i + C_];
        } else {
#pragma unroll
          for (int i = 0; i < (S_ - 2) * C_; ++i) xq[i] = xq[i + 2 * C_];
        }
        if (stride == 1) {
          constexpr int ss = S_ - 1;
          const int iw = iw0 + ss;
          const bool ok = (unsigned)iw < (unsigned)W;
          const T16* src = ok ? row + (long)iw * C_ : zpage;
#pragma unroll
          for (int c = 0; c < C_; ++c)
            xq[ss * C_ + c] = F16<T16>::to_f32(src[c]);
        } else {
#pragma unroll
          for (int jj = 0; jj < 2; ++jj) {
            const int ss = S_ - 2 + jj;
            const int iw = iw0 + ss;
            const bool ok = (unsigned)iw < (unsigned)W;
            const T16* src = ok ? row + (long)iw * C_ : zpage;
#pragma unroll
            for (int c = 0; c < C_; ++c)
              xq[ss * C_ + c] = F16<T16>::to_f32(src[c]);
          }
        }
      }
      const float dyv =
          (k < K) ? F16<T16>::to_f32(dy[m * K + k]) : 0.f;
      if (rok && dyv != 0.f) {
#pragma unroll
        for (int i = 0; i < S_ * C_; ++i) acc[i] += dyv * xq[i];
      }
      if (++q == Wo) {
        q = 0;
        fresh = true;
        if (++p == Ho) {
          p = 0;
          ++n;
        }
      }
    }
  }
  if (k < K) {
    const long E = (long)K * R * S_ * C_;
    float* slab = part + ((long)blockIdx.x * 4 + wv) * E;
#pragma unroll
    for (int s = 0; s < S_; ++s)
#pragma unroll
      for (int c = 0; c < C_; ++c)
        slab[(((long)k * C_ + c) * R + r) * S_ + s] = acc[s * C_ + c];
  }
}

}  // namespace

static inline int out_dim(int in, int k, int stride, int pad) {
  return (in + 2 * pad - k) / stride + 1;
}

// MFMA GEMM stems (stem_mfma.hip) replace the dot2 kernels; =0 disables
static bool stem_gemm_on() {
  static const bool v = EnvKnob("MI355X_STEM_GEMM").on();
  return v;
}

// conv_fwd_smallc<C_, S_>: the N*P*Q outputs in m-chunks, one per block
template <int C_, int S_>
static void fwd_smallc_launch(const at::Tensor& x, const at::Tensor& w,
                              const at::Tensor& bias, at::Tensor& y,
                              long stride, long pad, long act) {
  const int N = x.size(0), H = x.size(1), W = x.size(2);
  const int P = y.size(1), Q = y.size(2), K = y.size(3);
  const long M = (long)N * P * Q;
  const long wrow = w.dim() == 2 ? w.size(1) : (long)S_ * S_ * C_;
  const SplitPlan sp = split_plan(M, std::min<long>(2048, cdiv_l(M, 256)));
  const int has_bias = bias.numel() > 0;
  at::Tensor zp = conv_zero_page(x);
  DISPATCH_16(x, T16, {
    launch256(conv_fwd_smallc<T16, C_, S_>, dim3(sp.n), 0,
              (const T16*)x.data_ptr(), (const T16*)w.data_ptr(),
              has_bias ? bias.data_ptr<float>() : nullptr,
              (const T16*)zp.data_ptr(), (T16*)y.data_ptr(), N, H, W, K, P, Q,
              stride, pad, wrow, act, has_bias, sp.per, M);
  });
}

// conv_wgrad_smallc<C_, S_>: grid (m-chunks, filter rows), one partial slab
// per wave, folded by wgrad_reduce_launch
template <int C_, int S_>
static void wgrad_smallc_launch(const at::Tensor& x, const at::Tensor& dy,
                                at::Tensor& dw, int R, long stride,
                                long pad) {
  const int N = x.size(0), H = x.size(1), W = x.size(2);
  const int P = dy.size(1), Q = dy.size(2), K = dy.size(3);
  const long M = (long)N * P * Q;
  const long E = (long)K * R * S_ * C_;
  const SplitPlan sp = split_plan(
      M, std::min<long>(std::max<long>(2048 / R, 1), cdiv_l(M, 256)));
  // empty, not zeros: every slab element is written (acc starts at 0 and
  // the store runs even for waves with an empty m-range)
  auto part = at::empty({sp.n * 4, E}, x.options().dtype(at::kFloat));
  at::Tensor zp = conv_zero_page(x);
  DISPATCH_16(x, T16, {
    launch256(conv_wgrad_smallc<T16, C_, S_>, dim3((unsigned)sp.n, R), 0,
              (const T16*)x.data_ptr(), (const T16*)dy.data_ptr(),
              (const T16*)zp.data_ptr(), part.data_ptr<float>(), N, H, W, K,
              P, Q, R, stride, pad, sp.per, M);
  });
  wgrad_reduce_launch(part, dw, E, sp.n * 4);
}

// row-chunk plan of the LDS stem wgrads: 512 blocks x 4 waves at occupancy
// 2 fills the chip exactly once; fewer chunks = 4x less partial-slab
// traffic for the reduce
static SplitPlan stem_rows_plan(long nrows) {
  return split_plan(nrows, std::min<long>(512, nrows));
}

at::Tensor conv2d_fwd(at::Tensor x, at::Tensor w, at::Tensor bias,
                      long stride, long pad, long act, long kR, long kS) {
  CHECK_GPU(x);
  CHECK_CONTIG(x);
  CHECK_16BIT(x);
  CHECK_CONTIG(w);
  const int N = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  const int K = w.size(0);
  const int R = w.dim() == 4 ? w.size(1) : kR;
  const int S = w.dim() == 4 ? w.size(2) : kS;
  const int P = out_dim(H, R, stride, pad), Q = out_dim(W, S, stride, pad);
  auto y = at::empty({N, P, Q, K}, x.options());
  // dedicated ImageNet-stem kernel: 7x7/s2/C=3 (dot2-packed sliding rows)
  const bool stem7 = K <= 64 && C == 3 && R == 7 && S == 7 && stride == 2 &&
                     pad <= 3;
  if (stem7 && w.dim() == 2 && K % 64 == 0 && stem_gemm_on()) {
    conv_fwd_stem_gemm_launch(x, w, bias, y, pad, act, at::Tensor(), 7, 2);
    return y;
  }
  if (stem7) {
    const long wrow = w.dim() == 2 ? w.size(1) : (long)R * S * C;
    const int has_bias = bias.numel() > 0;
    const size_t smem = stem7_strip(Q, x.element_size()).bytes;
    DISPATCH_16(x, T16, {
      launch256(conv_fwd_stem7_lds<T16>, dim3((unsigned)(N * P)), smem,
                (const T16*)x.data_ptr(), (const T16*)w.data_ptr(),
                has_bias ? bias.data_ptr<float>() : nullptr,
                (T16*)y.data_ptr(), N, H, W, K, P, Q, pad, wrow, act,
                has_bias);
    });
    return y;
  }
  // CIFAR stem 3x3/s1 with K % 64 == 0 (dim-2 padded weight): MFMA GEMM
  // (stem_mfma.hip) — the dot2 LDS kernels below are the K < 64 fallback
  if (C == 3 && R == 3 && S == 3 && stride == 1 && pad <= 1 &&
      w.dim() == 2 && K % 64 == 0 && stem_gemm_on()) {
    conv_fwd_stem_gemm_launch(x, w, bias, y, pad, act, at::Tensor(), 3, 1);
    return y;
  }
  // CIFAR stem 3x3/s1/p1: LDS-staged variant (conv_fwd_stem3_lds)
  if (K <= 64 && C == 3 && R == 3 && S == 3 && stride == 1 && pad == 1 &&
      P == H && Q == W) {
    const long wrow = w.dim() == 2 ? w.size(1) : 27L;
    const size_t smem = stem3_strip(Q).bytes;
    const int has_bias = bias.numel() > 0;
    DISPATCH_16(x, T16, {
      launch256(conv_fwd_stem3_lds<T16>, dim3((unsigned)(N * P)), smem,
                (const T16*)x.data_ptr(), (const T16*)w.data_ptr(),
                has_bias ? bias.data_ptr<float>() : nullptr,
                (T16*)y.data_ptr(), N, H, W, K, P, Q, wrow, act, has_bias);
    });
    return y;
  }
  const bool smallc_fwd = K <= 64 && R == 3 && S == 3 && (C == 3 || C == 6) &&
                          (stride == 1 || stride == 2);
  if (smallc_fwd) {
    if (C == 3)
      fwd_smallc_launch<3, 3>(x, w, bias, y, stride, pad, act);
    else
      fwd_smallc_launch<6, 3>(x, w, bias, y, stride, pad, act);
    return y;
  }
  if (w.dim() == 2) {  // padded [KO,KGP] weight: generic small-C MFMA path
    conv_fwd_mfma_genc_launch(x, w, bias, y, R, S, stride, pad, act);
    return y;
  }
  TORCH_CHECK(w.size(3) == C, "conv weight/input channel mismatch");
  if (conv_mfma_supported(C, K)) {
    conv_fwd_mfma_launch(x, w, bias, y, stride, pad, act, at::Tensor(),
                         at::Tensor(), at::Tensor());
    return y;
  }
  const long total = (long)N * P * Q * K;
  const int has_bias = bias.numel() > 0;
  DISPATCH_16(x, T16, {
    launch256(conv_fwd_direct<T16>, conv_grid(total), 0,
              (const T16*)x.data_ptr(), (const T16*)w.data_ptr(),
              has_bias ? bias.data_ptr<float>() : nullptr, (T16*)y.data_ptr(),
              N, H, W, C, K, R, S, P, Q, stride, pad, act, has_bias);
  });
  return y;
}

// conv->BN fusion entry: returns {y, stats[2,C]} with stats computed in
// the conv epilogue (empty stats if this shape has no fusable path — the
// caller then runs the separate bn_stats pass). kR/kS: filter dims for
// dim-2 (pre-padded) weights, so the fallback dispatch stays correct.
std::vector<at::Tensor> conv2d_fwd_stats(at::Tensor x, at::Tensor w,
                                         long stride, long pad, long kR,
                                         long kS) {
  CHECK_GPU(x);
  CHECK_CONTIG(x);
  CHECK_16BIT(x);
  CHECK_CONTIG(w);
  const int N = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  const int K = w.size(0);
  // stems (C=3, dim-2 padded weight): 7x7/s2 ImageNet and 3x3/s1 CIFAR —
  // the strip kernel's epilogue can emit stats too
  if (w.dim() == 2 && C == 3 && K % 64 == 0 && stem_gemm_on() &&
      ((kR == 7 && kS == 7 && stride == 2 && pad <= 3) ||
       (kR == 3 && kS == 3 && stride == 1 && pad <= 1))) {
    const int P = out_dim(H, kR, stride, pad);
    const int Q = out_dim(W, kS, stride, pad);
    auto y = at::empty({N, P, Q, K}, x.options());
    auto stats = at::zeros({2, K}, x.options().dtype(at::kFloat));
    auto empty_bias = at::empty(0, x.options().dtype(at::kFloat));
    const bool got = conv_fwd_stem_gemm_launch(x, w, empty_bias, y, pad, 0,
                                               stats, kR, stride);
    return {y, got ? stats : at::Tensor()};
  }
  if (w.dim() != 4 || !conv_mfma_supported(C, K)) {
    auto empty_bias = at::empty(0, x.options().dtype(at::kFloat));
    auto y = conv2d_fwd(x, w, empty_bias, stride, pad, 0,
                        w.dim() == 4 ? w.size(1) : kR,
                        w.dim() == 4 ? w.size(2) : kS);
    return {y, at::Tensor()};
  }
  const int R = w.size(1), S = w.size(2);
  const int P = out_dim(H, R, stride, pad), Q = out_dim(W, S, stride, pad);
  auto y = at::empty({N, P, Q, K}, x.options());
  // empty, not zeros: the ordered slab fold stores every stats element
  auto stats = at::empty({2, K}, x.options().dtype(at::kFloat));
  auto empty_bias = at::empty(0, x.options().dtype(at::kFloat));
  conv_fwd_mfma_launch(x, w, empty_bias, y, stride, pad, 0, stats,
                       at::Tensor(), at::Tensor());
  return {y, stats};
}

// addin (optional, dx-shaped): dx = dgrad(dy) + addin — carries the
// residual-junction gradient of a ResNet block so autograd's separate
// full-tensor add at the junction disappears (MFMA path only).
// lazy-BN fused entry: z = relu(x*asc + ash) applied to the x operand on
// load (the BN apply pass and its output tensor never materialize);
// returns {y, stats[2,KO] or empty} (stats when want_stats, from the conv
// epilogue — feeds the NEXT BN).
std::vector<at::Tensor> conv2d_fwd_scaled(at::Tensor x, at::Tensor w,
                                          at::Tensor asc, at::Tensor ash,
                                          long stride, long pad,
                                          bool want_stats) {
  CHECK_GPU(x);
  CHECK_CONTIG(x);
  CHECK_16BIT(x);
  CHECK_CONTIG(w);
  const int N = x.size(0), H = x.size(1), W_ = x.size(2), C = x.size(3);
  const int K = w.size(0);
  TORCH_CHECK(w.dim() == 4 && conv_mfma_supported(C, K),
              "conv2d_fwd_scaled needs the MFMA path (C,K % 64 == 0)");
  const int R = w.size(1), S = w.size(2);
  const int P = out_dim(H, R, stride, pad), Q = out_dim(W_, S, stride, pad);
  auto y = at::empty({N, P, Q, K}, x.options());
  auto stats = want_stats
                   ? at::empty({2, K}, x.options().dtype(at::kFloat))
                   : at::Tensor();
  auto empty_bias = at::empty(0, x.options().dtype(at::kFloat));
  conv_fwd_mfma_launch(x, w, empty_bias, y, stride, pad, 0, stats, asc, ash);
  return {y, want_stats ? stats : at::Tensor()};
}

// lazy-BN wgrad: the x operand transformed on load like conv2d_fwd_scaled
at::Tensor conv2d_wgrad_scaled(at::Tensor x, at::Tensor asc, at::Tensor ash,
                               at::Tensor dy, long R, long S, long stride,
                               long pad) {
  CHECK_GPU(x);
  CHECK_CONTIG(x);
  CHECK_CONTIG(dy);
  const int C = x.size(3);
  const int K = dy.size(3);
  TORCH_CHECK(conv_mfma_supported(C, K),
              "conv2d_wgrad_scaled needs the MFMA path (C,K % 64 == 0)");
  auto dw = at::empty({(long)K, (long)C, R, S},
                      x.options().dtype(at::kFloat));
  conv_wgrad_mfma_launch(x, dy, dw, R, S, stride, pad, asc, ash);
  return dw;
}

at::Tensor conv2d_dgrad(at::Tensor dy, at::Tensor wflip, long stride,
                        long pad, long H, long W, at::Tensor addin) {
  CHECK_GPU(dy);
  CHECK_CONTIG(dy);
  CHECK_16BIT(dy);
  const int N = dy.size(0), P = dy.size(1), Q = dy.size(2), K = dy.size(3);
  const int R = wflip.size(0), S = wflip.size(1), C = wflip.size(2);
  auto dx = at::empty({N, H, W, (long)C}, dy.options());
  if (conv_mfma_supported(K, C)) {
    conv_dgrad_mfma_launch(dy, wflip, dx, R, S, stride, pad, addin);
    return dx;
  }
  TORCH_CHECK(!(addin.defined() && addin.numel() > 0),
              "addin requires the MFMA dgrad path (C,K % 64 == 0)");
  const long total = (long)N * H * W * C;
  DISPATCH_16(dy, T16, {
    launch256(conv_dgrad_direct<T16>, conv_grid(total), 0,
              (const T16*)dy.data_ptr(), (const T16*)wflip.data_ptr(),
              (T16*)dx.data_ptr(), N, H, W, C, K, R, S, P, Q, stride, pad);
  });
  return dx;
}

at::Tensor conv2d_wgrad(at::Tensor x, at::Tensor dy, long R, long S,
                        long stride, long pad) {
  CHECK_GPU(x);
  CHECK_CONTIG(x);
  CHECK_CONTIG(dy);
  const int N = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  const int P = dy.size(1), Q = dy.size(2), K = dy.size(3);
  const long M = (long)N * P * Q;
  const long total_w = (long)K * R * S * C;
  if (conv_mfma_supported(C, K)) {
    // empty, not zeros: the MFMA wgrad tiles cover every [K,C,R,S] element
    // with plain stores (nchunks==1) or via wgrad_reduce_chunks (nchunks>1)
    auto dw = at::empty({K, (long)C, R, S}, x.options().dtype(at::kFloat));
    conv_wgrad_mfma_launch(x, dy, dw, R, S, stride, pad, at::Tensor(),
                           at::Tensor());
    return dw;
  }
  if (K % 64 == 0 && C == 3 && R == 3 && S == 3 && stride == 1 &&
      pad <= 1 && stem_gemm_on()) {
    auto dw = at::empty({K, 3L, 3L, 3L}, x.options().dtype(at::kFloat));
    conv_wgrad_stem_gemm_launch(x, dy, dw, pad, 3, 1);
    return dw;
  }
  if (K <= 64 && C == 3 && R == 3 && S == 3 && stride == 1 && pad == 1 &&
      P == H && Q == W) {
    const SplitPlan rp = stem_rows_plan((long)N * P);
    const long E = (long)K * 27;
    auto dw = at::empty({K, 3L, 3L, 3L}, x.options().dtype(at::kFloat));
    auto partl = at::empty({rp.n * 4, E}, x.options().dtype(at::kFloat));
    const size_t smem = stem3_strip(Q).bytes + (size_t)Q * K * 2;
    DISPATCH_16(x, T16, {
      launch256(conv_wgrad_stem3_lds<T16>, dim3((unsigned)rp.n), smem,
                (const T16*)x.data_ptr(), (const T16*)dy.data_ptr(),
                partl.data_ptr<float>(), N, H, W, K, P, Q, rp.per);
    });
    wgrad_reduce_launch(partl, dw, E, rp.n * 4);
    return dw;
  }
  const bool smallc = K <= 64 &&
      ((C == 3 && (S == 3 || S == 5 || S == 7)) || (C == 6 && S == 5));
  if (smallc) {
    const long E = (long)K * R * S * C;
    auto dw = at::empty({K, (long)C, R, S}, x.options().dtype(at::kFloat));
    if (C == 3 && S == 7 && stride == 2 && pad <= 4) {
      if (K % 64 == 0 && R == 7 && pad <= 3 && stem_gemm_on()) {
        conv_wgrad_stem_gemm_launch(x, dy, dw, pad, 7, 2);
        return dw;
      }
      const SplitPlan rp = stem_rows_plan((long)N * P);
      auto partl = at::empty({rp.n * 4, E}, x.options().dtype(at::kFloat));
      const size_t smem = stem7_strip(Q, 4).bytes + (size_t)Q * K * 2;
      DISPATCH_16(x, T16, {
        launch256(conv_wgrad_stem7_lds<T16>, dim3((unsigned)rp.n), smem,
                  (const T16*)x.data_ptr(), (const T16*)dy.data_ptr(),
                  partl.data_ptr<float>(), N, H, W, K, P, Q, pad, rp.per);
      });
      wgrad_reduce_launch(partl, dw, E, rp.n * 4);
      return dw;
    }
    if (C == 3 && S == 3)
      wgrad_smallc_launch<3, 3>(x, dy, dw, R, stride, pad);
    else if (C == 3 && S == 5)
      wgrad_smallc_launch<3, 5>(x, dy, dw, R, stride, pad);
    else if (C == 3 && S == 7)
      wgrad_smallc_launch<3, 7>(x, dy, dw, R, stride, pad);
    else
      wgrad_smallc_launch<6, 5>(x, dy, dw, R, stride, pad);
    return dw;
  }
  // split the NPQ reduction so small filters still fill the chip
  int nchunks = (int)std::min<long>(cdiv_l(M, 1024),
                                    std::max<long>(1, (256L * 8192) / std::max(total_w, 1L)));
  nchunks = std::max(nchunks, 1);
  const long m_per_chunk = cdiv_l(M, nchunks);
  auto dw = at::empty({K, (long)C, R, S}, x.options().dtype(at::kFloat));
  auto part = nchunks == 1
                  ? dw
                  : at::empty({nchunks, total_w}, x.options().dtype(at::kFloat));
  dim3 grid((unsigned)std::min<long>(cdiv_l(total_w, 256), 4096), nchunks);
  DISPATCH_16(x, T16, {
    launch256(conv_wgrad_direct<T16>, grid, 0, (const T16*)x.data_ptr(),
              (const T16*)dy.data_ptr(), part.data_ptr<float>(), N, H, W, C,
              K, R, S, P, Q, stride, pad, m_per_chunk);
  });
  if (nchunks > 1) fold_rows(part, dw, total_w, nchunks);
  return dw;
}
