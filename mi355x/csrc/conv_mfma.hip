// MFMA implicit-GEMM conv for CDNA4 (gfx950) — the hot path for every
// ResNet conv (C%64==0, K%64==0). One gather-GEMM kernel serves forward
// (TRANS=false) and dgrad (TRANS=true; host pre-flips the weight to
// [R,S,C,K] so dgrad is the same GEMM with transposed-window gather).
//
// GEMM view: OUT[M=N*Ho*Wo, KO] = A[M, R*S*CI] * B,
// iterated as (r,s,c-chunk) k-slices of BK=64. A k-slice of A is a
// contiguous 64-channel read of the input window row (NHWC), staged
// through registers into LDS with zero-fill for padding/out-of-window
// rows (predication the glds path can't do). Structure follows the
// canonical CDNA GEMM anatomy (cdna_hip_programming.md §5): 128x64 block
// tile, 4 waves x (32M x 64N) each as 2 x mfma_f32_32x32x16, LDS tiles
// [row][BK+8] padded against bank conflicts (G4), T14-style staging
// (write after barrier, next global load issued under the MFMA phase).
//
// Epilogue (conv_epilogue.h): the accumulator has the output channel on
// the lane and the row in the register, which stored directly is 2 bytes
// per lane. conv_gather_gemm, conv_dgrad_s2_gemm and the ADDIN variant of
// conv_patch_gemm instead stage the rounded tile in the A/B (or patch) LDS
// the main loop is done with and write whole output rows, 16 bytes per
// lane; a residual ADDIN tile is read the same way. For that their B rows
// are staged in the order epi_brow gives, so that a lane's NT values are
// adjacent channels. The plain conv_patch_gemm variants keep the direct
// store: their stores already hide behind the next blocks' patch fill, and
// the extra barrier and LDS round trip measured 2% slower
// (profiles/r04_conv_epilogue.md).
#include "conv_epilogue.h"
#include "conv_internal.h"

typedef __attribute__((ext_vector_type(8))) _Float16 half8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

namespace {

template <typename T16>
struct Mfma32 {};
template <>
struct Mfma32<__hip_bfloat16> {
  static DEV_INLINE f32x16 run(short8 a, short8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
};
template <>
struct Mfma32<__half> {
  static DEV_INLINE f32x16 run(short8 a, short8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16((half8)a, (half8)b, c, 0, 0,
                                                  0);
  }
};

// lazy-BN A-side transform: z = relu(x*sc + sh) applied to an 8-channel
// group in registers at load/stage time (the normalized activation is
// never materialized; the VALU rides under the MFMA phase). Scale/shift
// come in as four float4 REGISTERS — v1 indexed asc[c0+u] per element
// (64 scalar L1 loads per thread per k-step) and measured -10% end to
// end from load-issue bloat alone.
struct Sc8 {
  float4v s0, s1, h0, h1;
};

DEV_INLINE Sc8 sc8_load(const float* __restrict__ asc,
                        const float* __restrict__ ash, int c) {
  Sc8 r;
  r.s0 = *reinterpret_cast<const float4v*>(asc + c);
  r.s1 = *reinterpret_cast<const float4v*>(asc + c + 4);
  r.h0 = *reinterpret_cast<const float4v*>(ash + c);
  r.h1 = *reinterpret_cast<const float4v*>(ash + c + 4);
  return r;
}

template <typename T16>
DEV_INLINE short8 scale8(short8 v, const Sc8& sc) {
  short8 o;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const float f = s16_to_f32<T16>(v[u]) * sc.s0[u] + sc.h0[u];
    o[u] = f32_to_s16<T16>(relu_f(f));
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const float f = s16_to_f32<T16>(v[4 + u]) * sc.s1[u] + sc.h1[u];
    o[4 + u] = f32_to_s16<T16>(relu_f(f));
  }
  return o;
}

constexpr int BM = 128, BN = 64, BK = 64;
constexpr int LDK = BK + 8;  // +16B pad: spreads fragment reads over banks
// NT = 32-wide N(output-channel) tiles per block: 2 (BN=64) or 4 (BN=128);
// wider tiles double the MFMA work per barrier pair for the K>=128 layers

// TRANS=false (fwd): src row = ho*stride - pad + r, in [0,Hi)
// TRANS=true (dgrad): src row = (ho + pad - r), valid iff %stride==0, /stride in [0,Hi)
// GENC (fwd only): CI % 64 != 0 — the weight is pre-padded to
// [KO, KGP=ceil(R*S*CI/64)*64] with kg=(r*S+s)*CI+c and zeros beyond, and
// the A side gathers per-ELEMENT across tap boundaries (stem convs C=3/6).
// ADDIN (compile-time — a runtime addin branch in this shared epilogue
// measurably slowed the non-addin convs): out += addin elementwise, the
// residual-junction gradient fused into the dgrad epilogue.
template <typename T16, bool TRANS, bool GENC, int NT, bool ADDIN = false,
          bool SCALED = false>
// min-blocks hint: same effect as on the wgrad kernel (see comment there)
__global__ __launch_bounds__(256, 2) void conv_gather_gemm(
    const T16* __restrict__ in,    // [N, Hi, Wi, CI]
    const T16* __restrict__ wgt,   // fwd: [KO, R*S*CI]; dgrad: [R*S, CI... ] via strides
    const float* __restrict__ bias,  // [KO] or null
    const T16* __restrict__ zpage,   // >=256 zero elements (OOB gather target)
    const T16* __restrict__ addin,   // ADDIN only: same layout as out
    const float* __restrict__ asc,   // SCALED only: [CI] scale
    const float* __restrict__ ash,   // SCALED only: [CI] shift
    T16* __restrict__ out,         // [N*Ho*Wo, KO]
    float* __restrict__ stats_slab,  // null, or [gy][gx][2][BNT] partial
    const int N, const int Hi, const int Wi, const int CI, const int KO,  //  (sum,sumsq) of this block's output tile (conv->BN fusion)
    const int Ho, const int Wo, const int R, const int S, const int stride,
    const int pad, const long b_row_stride, const long b_rs_stride,
    const int act, const int has_bias) {
  // single-buffered: 2x LDS for a double buffer measurably LOSES here —
  // it halves blocks/CU and the cross-block overlap it sacrifices was
  // already hiding the staging latency (guide common-mistake #5)
  __shared__ T16 lds[BM * LDK + NT * 32 * LDK];

  const int tid = threadIdx.x;
  const long Mtot = (long)N * Ho * Wo;
  const long bm0 = (long)blockIdx.x * BM;
  constexpr int BNT = NT * 32;
  const int k0 = blockIdx.y * BNT;

  // ---- A staging coords (2 threads per m-row, 32 channels each) ----
  const int sa_m = tid >> 1;
  const int sa_c = (tid & 1) * (BK / 2);
  const long m_a = bm0 + sa_m;
  const bool m_ok = m_a < Mtot;
  int n_ = 0, p_ = 0, q_ = 0;
  if (m_ok) {
    n_ = (int)(m_a / ((long)Ho * Wo));
    const int pq = (int)(m_a % ((long)Ho * Wo));
    p_ = pq / Wo;
    q_ = pq % Wo;
  }
  // fwd: top-left of the receptive field; dgrad: p_,q_ used directly
  const int ih0 = TRANS ? p_ : p_ * stride - pad;
  const int iw0 = TRANS ? q_ : q_ * stride - pad;

  // ---- B staging coords (256/BNT threads per n-row) ----
  constexpr int TPR = 256 / BNT;          // threads per B row
  constexpr int EPT = BK / TPR;           // elements per thread
  const int sb_n = tid / TPR;
  const int sb_c = (tid % TPR) * EPT;
  const T16* wrow = wgt + (long)(k0 + sb_n) * b_row_stride + sb_c;

  // ---- wave/lane fragment coords ----
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int li = lane & 31;
  const int kh = lane >> 5;  // k-half: lane holds k = kk + kh*8 + e
  const int wm = wave * 32;  // wave's m-offset inside the block tile

  f32x16 acc[NT] = {};

  const int cchunks = GENC ? 1 : CI / BK;
  const int ksteps = GENC ? (int)(b_row_stride / BK)  // KGP/64
                          : R * S * cchunks;

  short8 sa[4];            // 32 channels = 4 x 16B
  short8 sb[EPT / 8];      // B elements per thread

  auto load_step_genc = [&](int j) {
    // per-element gather: kg walks (tap, c) with carries (fully unrolled,
    // so the vector-register indices stay compile-time — guide rule 20)
    const int kg0 = j * BK + sa_c;
    int tap = kg0 / CI;
    int c = kg0 - tap * CI;
    int r_ = tap / S;
    int s_ = tap - r_ * S;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      const int ih = ih0 + r_;
      const int iw = iw0 + s_;
      const bool ok = m_ok && tap < R * S && (unsigned)ih < (unsigned)Hi &&
                      (unsigned)iw < (unsigned)Wi;
      // address select, not a branch: keeps all 32 loads unconditional so
      // they batch under one wait instead of 32 serialized round trips
      const T16* src =
          ok ? in + (((long)n_ * Hi + ih) * Wi + iw) * CI + c : zpage + i;
      short val;
      const T16 v = *src;
      __builtin_memcpy(&val, &v, 2);
      sa[i / 8][i % 8] = val;
      if (++c == CI) {
        c = 0;
        ++tap;
        if (++s_ == S) {
          s_ = 0;
          ++r_;
        }
      }
    }
    const T16* wp = wgt + (long)(k0 + sb_n) * b_row_stride + j * BK + sb_c;
#pragma unroll
    for (int i = 0; i < EPT / 8; ++i)
      sb[i] = *reinterpret_cast<const short8*>(wp + 8 * i);
  };

  // incremental (c-chunk, s, r) decode — load_step is called exactly once
  // per j in order, so three runtime divisions per k-step reduce to carry
  // counters (same lever as the wgrad kernels' m-decode). The per-tap
  // position (validity + image offset, incl. the TRANS stride div/mod
  // pair) is CACHED and recomputed only when the tap advances — for a
  // 1x1 dgrad the whole k-loop walks c-chunks of one tap.
  int cc_i = 0, s_i = 0, r_i = 0;
  bool va_tap = m_ok;
  long ioff_tap = 0;
  auto load_step = [&](int j) {
    if constexpr (GENC) {
      load_step_genc(j);
      return;
    }
    (void)j;
    const int c0 = cc_i * BK;
    const int s_ = s_i;
    const int r_ = r_i;
    if (cc_i == 0) {  // first chunk of this tap: refresh the position
      bool va = m_ok;
      long ioff = 0;
      if constexpr (TRANS) {
        const int ph = ih0 + pad - r_;
        const int qw = iw0 + pad - s_;
        const int pp = ph / stride, qq = qw / stride;
        va = va && ph >= 0 && qw >= 0 && (ph % stride) == 0 &&
             (qw % stride) == 0 && pp < Hi && qq < Wi;
        if (va) ioff = (((long)n_ * Hi + pp) * Wi + qq) * CI;
      } else {
        const int ih = ih0 + r_;
        const int iw = iw0 + s_;
        va = va && (unsigned)ih < (unsigned)Hi && (unsigned)iw < (unsigned)Wi;
        if (va) ioff = (((long)n_ * Hi + ih) * Wi + iw) * CI;
      }
      va_tap = va;
      ioff_tap = ioff;
    }
    if (++cc_i == cchunks) {
      cc_i = 0;
      if (++s_i == S) {
        s_i = 0;
        ++r_i;
      }
    }
    const bool va = va_tap;
    const long ioff = ioff_tap;
    const T16* xp = va ? in + ioff + c0 + sa_c : zpage;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      sa[i] = *reinterpret_cast<const short8*>(xp + (va ? 8 * i : 0));
    if constexpr (SCALED) {
      if (va) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          sa[i] = scale8<T16>(sa[i],
                              sc8_load(asc, ash, c0 + sa_c + 8 * i));
      }
    }
    const T16* wp = wrow + (long)(r_ * S + s_) * b_rs_stride + c0;
#pragma unroll
    for (int i = 0; i < EPT / 8; ++i)
      sb[i] = *reinterpret_cast<const short8*>(wp + 8 * i);
  };

  auto stage = [&]() {
    T16* ldsA = lds;
    T16* ldsB = lds + BM * LDK;
    short* pa = reinterpret_cast<short*>(ldsA + sa_m * LDK + sa_c);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<short8*>(pa + 8 * i) = sa[i];
    short* pb =
        reinterpret_cast<short*>(ldsB + epi_brow<NT>(sb_n) * LDK + sb_c);
#pragma unroll
    for (int i = 0; i < EPT / 8; ++i)
      *reinterpret_cast<short8*>(pb + 8 * i) = sb[i];
  };

  load_step(0);
  for (int j = 0; j < ksteps; ++j) {
    __syncthreads();  // previous MFMA phase done reading LDS
    stage();
    __syncthreads();
    if (j + 1 < ksteps) load_step(j + 1);  // overlaps the MFMA phase
    const T16* ldsA = lds;
    const T16* ldsB = lds + BM * LDK;
#pragma unroll
    for (int kk = 0; kk < BK; kk += 16) {
      const short8 af = *reinterpret_cast<const short8*>(
          ldsA + (wm + li) * LDK + kk + kh * 8);
#pragma unroll
      for (int tnt = 0; tnt < NT; ++tnt) {
        const short8 bf = *reinterpret_cast<const short8*>(
            ldsB + (tnt * 32 + li) * LDK + kk + kh * 8);
        acc[tnt] = Mfma32<T16>::run(af, bf, acc[tnt]);
      }
    }
  }

  // ---- epilogue: bias + act (+ optional BN-stats partials) in fp32
  // registers, one rounding, then whole-row 16-byte stores through the
  // wave's LDS region (conv_epilogue.h; lane li holds channels li*NT+t) ----
  using E = EpiTile<NT>;
  static_assert(sizeof(lds) >= E::BYTES, "epilogue tile must fit the A/B LDS");
  short* wl = reinterpret_cast<short*>(lds) + wave * E::WAVE;
  long roff[E::NIT];
#pragma unroll
  for (int it = 0; it < E::NIT; ++it) {
    const long m = bm0 + wm + epi_io_row<NT>(it, lane);
    roff[it] = m < Mtot ? m * KO + k0 : -1;
  }
  __syncthreads();  // every wave's last MFMA phase is done reading LDS
  if constexpr (ADDIN) {
    epi_fetch<T16, NT>(wl, addin, lane, roff);
    epi_wave_sync();
  }
  float bv[NT];
  float ssum[NT] = {}, ssq[NT] = {};
#pragma unroll
  for (int tnt = 0; tnt < NT; ++tnt)
    bv[tnt] = has_bias ? bias[k0 + li * NT + tnt] : 0.f;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int row = epi_acc_row(reg, kh);
    typename EpiPack<NT>::type h = {};
    if (bm0 + wm + row < Mtot) {
      if constexpr (ADDIN) h = epi_get<NT>(wl, row, li);
#pragma unroll
      for (int tnt = 0; tnt < NT; ++tnt) {
        float v = acc[tnt][reg] + bv[tnt];
        if constexpr (ADDIN) v += s16_to_f32<T16>(h[tnt]);
        if (act == 1) v = relu_f(v);
        if (stats_slab) {
          ssum[tnt] += v;
          ssq[tnt] += v * v;
        }
        h[tnt] = f32_to_s16<T16>(v);
      }
    }
    epi_put<NT>(wl, row, li, h);
  }
  epi_wave_sync();
  epi_flush<T16, NT>(wl, out, lane, roff);
  if (stats_slab) {
    // conv->BN fusion: fold the block's per-lane channel partials (8
    // lanes per channel: 4 waves x 2 kh halves) — kh halves via one
    // cross-lane xor-shuffle, waves via per-wave LDS rows summed by the
    // storing threads. (LDS float atomicAdd here measured ~3.7 us/block
    // of serialized conflicts — 50% on the whole patch kernel.)
    constexpr int BNTC = NT * 32;
#pragma unroll
    for (int tnt = 0; tnt < NT; ++tnt) {
      ssum[tnt] += __shfl_xor(ssum[tnt], 32, 64);
      ssq[tnt] += __shfl_xor(ssq[tnt], 32, 64);
    }
    float* lsum = reinterpret_cast<float*>(lds);  // [4 waves][2*BNTC]
    __syncthreads();  // the staged tiles (same LDS) have been read back
    if (kh == 0) {
#pragma unroll
      for (int tnt = 0; tnt < NT; ++tnt) {
        lsum[wave * 2 * BNTC + li * NT + tnt] = ssum[tnt];
        lsum[wave * 2 * BNTC + BNTC + li * NT + tnt] = ssq[tnt];
      }
    }
    __syncthreads();
    float* slab =
        stats_slab + ((long)blockIdx.y * gridDim.x + blockIdx.x) * 2 * BNTC;
    for (int t = tid; t < 2 * BNTC; t += 256)
      slab[t] = lsum[t] + lsum[2 * BNTC + t] + lsum[4 * BNTC + t] +
                lsum[6 * BNTC + t];
  }
}

// L1 of the two-level slab fold: plain partial sums over a gx-slice
// (large-M convs have 10k-65k slab rows; a single 64-block reduce over
// them measured 139 us latency-bound — this level keeps the chip full)
__global__ void conv_stats_partial(const float* __restrict__ slab,
                                   float* __restrict__ out, int gx, int bnt2,
                                   int bpb) {
  const int by = blockIdx.y;
  const int t = threadIdx.x;
  if (t >= bnt2) return;
  const int b0 = blockIdx.x * bpb;
  const int b1 = min(gx, b0 + bpb);
  float acc = 0.f;
  for (int bx = b0; bx < b1; ++bx)
    acc += slab[((long)by * gx + bx) * bnt2 + t];
  out[((long)by * gridDim.x + blockIdx.x) * bnt2 + t] = acc;
}

// stats[2][C] = sum over gx of slab[gy][gx][2][BNT]; one block per by
// sums the (at most 64) remaining rows in order — plain stores, so the
// statistics repeat bit for bit (no float atomics)
__global__ void conv_stats_reduce(const float* __restrict__ slab,
                                  float* __restrict__ stats, int gx, int bnt2,
                                  int C, int bx_per_block) {
  const int by = blockIdx.y;
  const int t = threadIdx.x;
  if (t >= bnt2) return;
  float acc = 0.f;
  const int b0 = blockIdx.x * bx_per_block;
  const int b1 = min(gx, b0 + bx_per_block);
  for (int bx = b0; bx < b1; ++bx)
    acc += slab[((long)by * gx + bx) * bnt2 + t];
  const int bnt = bnt2 / 2;
  const int h = t / bnt;
  const int c = by * bnt + (t % bnt);
  stats[h * C + c] = acc;  // launched with gridDim.x == 1
}

// stride-2 dgrad, parity-specialized: dx positions partition by
// (ih%2, iw%2) and each class only has contributions from taps of
// matching parity ((ih+pad-r) % 2 == 0), so the k-loop runs
// |Ra|*|Sa|*cchunks steps instead of R*S*cchunks. The plain TRANS gather
// wastes ~75% of its staging+MFMA on parity-invalid (all-zero) slices
// for 3x3/s2, and ALL of it for 3 of the 4 classes of a 1x1/s2
// downsample (those classes here just store zeros). ADDIN as in
// conv_gather_gemm (residual-tap fusion).
template <typename T16, int NT, bool ADDIN = false>
__global__ __launch_bounds__(256, 2) void conv_dgrad_s2_gemm(
    const T16* __restrict__ dy,     // [N, P, Q, KO]
    const T16* __restrict__ wflip,  // [R, S, CI, KO]
    const T16* __restrict__ zpage,
    const T16* __restrict__ addin,  // ADDIN only: dx-shaped
    T16* __restrict__ dx,           // [N, H, W, CI]
    const int N, const int P, const int Q, const int KO, const int CI,
    const int H, const int W, const int R, const int S, const int pad) {
  __shared__ T16 lds[BM * LDK + NT * 32 * LDK];
  const int tid = threadIdx.x;
  const int pa = blockIdx.z >> 1;  // ih % 2
  const int pb = blockIdx.z & 1;   // iw % 2
  const int Ha = (H - pa + 1) >> 1;
  const int Wa = (W - pb + 1) >> 1;
  const long Mc = (long)N * Ha * Wa;
  const long bm0 = (long)blockIdx.x * BM;
  constexpr int BNT = NT * 32;
  const int k0 = blockIdx.y * BNT;  // dx channel tile

  const int r0 = (pa + pad) & 1;  // r parity for this class
  const int s0 = (pb + pad) & 1;
  const int nr = r0 < R ? ((R - r0 + 1) >> 1) : 0;
  const int ns = s0 < S ? ((S - s0 + 1) >> 1) : 0;
  const int cchunks = KO / BK;
  const int ksteps = nr * ns * cchunks;

  const int sa_m = tid >> 1;
  const int sa_c = (tid & 1) * (BK / 2);
  const long m_a = bm0 + sa_m;
  const bool m_ok = m_a < Mc;
  int n_ = 0, ih_ = 0, iw_ = 0;
  if (m_ok) {
    n_ = (int)(m_a / ((long)Ha * Wa));
    const int rem = (int)(m_a % ((long)Ha * Wa));
    ih_ = 2 * (rem / Wa) + pa;
    iw_ = 2 * (rem % Wa) + pb;
  }

  constexpr int TPR = 256 / BNT;
  constexpr int EPT = BK / TPR;
  const int sb_n = tid / TPR;
  const int sb_c = (tid % TPR) * EPT;

  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int li = lane & 31;
  const int kh = lane >> 5;
  const int wm = wave * 32;
  f32x16 acc[NT] = {};
  short8 sa[4], sb[EPT / 8];

  // incremental (c-chunk, s, r) decode: runtime divisions per k-step
  // measured as 38% issue-stall (PMC) in this short-k kernel
  int cc_i = 0, s_i = 0, r_i = 0;
  bool va_tap = false;
  long ioff_tap = 0, woff_tap = 0;
  auto load_step = [&](int j) {
    (void)j;
    const int c0 = cc_i * BK;
    if (cc_i == 0) {  // first chunk of this tap: refresh the position
      const int s_ = s0 + 2 * s_i;
      const int r_ = r0 + 2 * r_i;
      const int dh = ih_ + pad - r_;  // even by construction
      const int dw_ = iw_ + pad - s_;
      const int pp = dh >> 1, qq = dw_ >> 1;
      va_tap = m_ok && dh >= 0 && dw_ >= 0 && pp < P && qq < Q;
      ioff_tap = (((long)n_ * P + pp) * Q + qq) * KO;
      woff_tap = ((long)r_ * S + s_) * CI * (long)KO;
    }
    if (++cc_i == cchunks) {
      cc_i = 0;
      if (++s_i == ns) {
        s_i = 0;
        ++r_i;
      }
    }
    const bool va = va_tap;
    const T16* xp = va ? dy + ioff_tap + c0 + sa_c : zpage;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      sa[i] = *reinterpret_cast<const short8*>(xp + (va ? 8 * i : 0));
    const T16* wp = wflip + woff_tap + (long)(k0 + sb_n) * KO + c0 + sb_c;
#pragma unroll
    for (int i = 0; i < EPT / 8; ++i)
      sb[i] = *reinterpret_cast<const short8*>(wp + 8 * i);
  };
  auto stage = [&]() {
    T16* ldsA = lds;
    T16* ldsB = lds + BM * LDK;
    short* pa_ = reinterpret_cast<short*>(ldsA + sa_m * LDK + sa_c);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<short8*>(pa_ + 8 * i) = sa[i];
    short* pb_ =
        reinterpret_cast<short*>(ldsB + epi_brow<NT>(sb_n) * LDK + sb_c);
#pragma unroll
    for (int i = 0; i < EPT / 8; ++i)
      *reinterpret_cast<short8*>(pb_ + 8 * i) = sb[i];
  };

  if (ksteps > 0) {
    load_step(0);
    for (int j = 0; j < ksteps; ++j) {
      __syncthreads();
      stage();
      __syncthreads();
      if (j + 1 < ksteps) load_step(j + 1);
      const T16* ldsA = lds;
      const T16* ldsB = lds + BM * LDK;
#pragma unroll
      for (int kk = 0; kk < BK; kk += 16) {
        const short8 af = *reinterpret_cast<const short8*>(
            ldsA + (wm + li) * LDK + kk + kh * 8);
#pragma unroll
        for (int tnt = 0; tnt < NT; ++tnt) {
          const short8 bf = *reinterpret_cast<const short8*>(
              ldsB + (tnt * 32 + li) * LDK + kk + kh * 8);
          acc[tnt] = Mfma32<T16>::run(af, bf, acc[tnt]);
        }
      }
    }
  }

  // epilogue: scatter into the strided class positions of dx. A row's
  // channels are contiguous, so rows leave as 16-byte pieces through the
  // wave's LDS region (conv_epilogue.h). One image-decode per lane; per
  // moved row only a rem-walk + one div by Wa (per-row /(Ha*Wa) pairs
  // were half of this kernel's issue stalls)
  using E = EpiTile<NT>;
  static_assert(sizeof(lds) >= E::BYTES, "epilogue tile must fit the A/B LDS");
  short* wl = reinterpret_cast<short*>(lds) + wave * E::WAVE;
  const long m_base = bm0 + wm;
  const int HaWa = Ha * Wa;
  int nn0 = 0, rem0 = 0;
  if (m_base < Mc) {
    nn0 = (int)(m_base / HaWa);
    rem0 = (int)(m_base % HaWa);
  }
  long roff[E::NIT];
#pragma unroll
  for (int it = 0; it < E::NIT; ++it) {
    const int row = epi_io_row<NT>(it, lane);
    roff[it] = -1;
    if (m_base + row < Mc) {
      int nn = nn0, rem = rem0 + row;
      while (rem >= HaWa) {
        rem -= HaWa;
        ++nn;
      }
      const int ih = 2 * (rem / Wa) + pa;
      const int iw = 2 * (rem - (rem / Wa) * Wa) + pb;
      roff[it] = (((long)nn * H + ih) * W + iw) * CI + k0;
    }
  }
  __syncthreads();  // every wave's last MFMA phase is done reading LDS
  if constexpr (ADDIN) {
    epi_fetch<T16, NT>(wl, addin, lane, roff);
    epi_wave_sync();
  }
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int row = epi_acc_row(reg, kh);
    typename EpiPack<NT>::type h = {};
    if constexpr (ADDIN) h = epi_get<NT>(wl, row, li);
#pragma unroll
    for (int tnt = 0; tnt < NT; ++tnt) {
      float v = acc[tnt][reg];
      if constexpr (ADDIN) v += s16_to_f32<T16>(h[tnt]);
      h[tnt] = f32_to_s16<T16>(v);
    }
    epi_put<NT>(wl, row, li, h);
  }
  epi_wave_sync();
  epi_flush<T16, NT>(wl, dx, lane, roff);
}

}  // namespace

// fold slab [by][gx][bnt2] -> stats[2,C]; partial levels (plain sums into
// fewer rows) until at most 64 rows are left for the single final block
// (external linkage: the stem kernels reuse it)
void stats_slab_reduce(at::Tensor slab, at::Tensor stats, int gx, int bnt2,
                       int C) {
  const int by = (int)(slab.numel() / ((long)gx * bnt2));
  if (gx > 4096) {
    const int bpb1 = (int)cdiv_l(gx, 1024);
    const int gx2 = (int)cdiv_l(gx, bpb1);
    auto l2 = at::empty({(long)by * gx2 * bnt2}, slab.options());
    launch256(conv_stats_partial, dim3(gx2, by), 0, slab.data_ptr<float>(),
              l2.data_ptr<float>(), gx, bnt2, bpb1);
    slab = l2;
    gx = gx2;
  }
  if (gx > 64) {
    const int bpb2 = (int)cdiv_l(gx, 64);
    const int gx3 = (int)cdiv_l(gx, bpb2);
    auto l3 = at::empty({(long)by * gx3 * bnt2}, slab.options());
    launch256(conv_stats_partial, dim3(gx3, by), 0, slab.data_ptr<float>(),
              l3.data_ptr<float>(), gx, bnt2, bpb2);
    slab = l3;
    gx = gx3;
  }
  launch256(conv_stats_reduce, dim3(1, by), 0, slab.data_ptr<float>(),
            stats.data_ptr<float>(), gx, bnt2, C, gx);
}

// ---------------------------------------------------------------------------
// ---------------------------------------------------------------------------
// Patch gather-GEMM for 3x3/stride-1/pad-1 (fwd and dgrad): the geometric
// input patch covering a 64-output tile (its q-rows +- 1 halo row, with
// zeroed pad columns) is staged into LDS ONCE per c-chunk; all NINE taps
// read it by address offset — the per-k-step global re-gather of the
// plain kernel (9x input traffic, 18 barriers/c-chunk) becomes one
// cooperative stage + 2 barriers. The B (weight) fragments live in
// REGISTERS, prefetched one tap ahead straight from L2 — no B tile in
// LDS, no B barriers. Vertical pad / image-crossing / M-tail are handled
// by a per-(lane, tap-row) address select onto a zeroed LDS stub (never a
// branch around the read).
//   block: 128m x 64k; 4 waves each own 32 m-rows x the full 64 k as TWO
//   32x32 acc tiles — one tile per wave makes every MFMA a serial
//   16-cycle dependency chain (measured 260-290 TF); two interleave to
//   the 8-cycle cadence.
//   patch: [NR rows][Wi+2 cols][72] (stride 72: 16B-aligned b128 reads,
//   36-dword lane stride -> worst 2-way bank conflicts).
//   epilogue: the plain variants store one 16-bit element per lane from
//   the accumulator. The ADDIN variant (dgrad + residual gradient) reads
//   the addin tile with 16-byte loads into the patch LDS, adds in fp32
//   registers, rounds once and writes whole rows with 16-byte stores
//   (conv_epilogue.h): 32 ushort loads + 32 short stores per wave become
//   4 + 4 dwordx4, and the kernel runs 20% faster. The same row store on
//   the plain variants measured 2% slower, so they do not use it.
// ---------------------------------------------------------------------------
constexpr int PCS = 72;  // patch col stride (elements)

template <typename T16, bool TRANS, bool ADDIN = false, bool SCALED = false>
__global__ __launch_bounds__(256, 2) void conv_patch_gemm(
    const T16* __restrict__ in,   // [N, Hi, Wi, CI] (dgrad: dy, CI=KO)
    const T16* __restrict__ wgt,  // fwd: [KO, 9*CI]; dgrad: wflip strides
    const float* __restrict__ bias,
    const T16* __restrict__ addin,  // ADDIN only: out += addin
    const float* __restrict__ asc,  // SCALED only: [CI] lazy-BN scale
    const float* __restrict__ ash,  // SCALED only: [CI] lazy-BN shift
    T16* __restrict__ out,
    float* __restrict__ stats_slab,  // null, or per-block (sum,sumsq) rows
    const int N, const int Hi, const int Wi, const int CI, const int KO,
    const long b_row_stride, const long b_rs_stride, const int act,
    const int has_bias, const int NR) {
  // whole-row epilogue store (conv_epilogue.h) for the ADDIN variant only
  constexpr bool ROWST = ADDIN;
  extern __shared__ __attribute__((aligned(16))) char psmem[];
  T16* patch = reinterpret_cast<T16*>(psmem);
  T16* zstub = patch + (long)NR * (Wi + 2) * PCS;  // 72 zero elements
  T16* ldsB = zstub + PCS;  // [64][LDK] weight tile for the current tap

  const int tid = threadIdx.x;
  const long Mtot = (long)N * Hi * Wi;  // Ho==Hi, Wo==Wi (s1p1)
  const int Wo = Wi, Ho = Hi;
  const long bm0 = (long)blockIdx.x * 128;
  const int k0 = blockIdx.y * 64;
  const long gr0 = bm0 / Wo - 1;  // first staged global row (n*Ho + p)

  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int li = lane & 31;
  const int kh = lane >> 5;
  const int wm = wave * 32;  // wave's m-rows (full 64 k per wave)

  // per-lane A-row coordinates (fixed across the whole kernel)
  const long m_lane = bm0 + wm + li;
  const long grl = m_lane / Wo;
  const int p_lane = (int)(grl % Ho);
  const int prow = (int)(grl - gr0);
  const int pcol = (int)(m_lane - grl * Wo) + 1;
  const bool m_ok = m_lane < Mtot;
  const long lane_base = ((long)prow * (Wi + 2) + pcol) * PCS;

  if (tid < 64) zstub[tid] = T16{};  // first barrier publishes it

  const int cchunks = CI / BK;
  f32x16 acc[2] = {};

  // B staged through LDS, cooperatively and COALESCED (per-lane scattered
  // weight-row loads measured 86.6% WAIT_ANY — a wave's worth of strided
  // 64B reads with 1-tap prefetch never hides L2 latency; the block-wide
  // burst + barrier pipeline does). 4 threads per B row, 16 elements each.
  const int sb_n = tid >> 2;
  const int sb_c = (tid & 3) * 16;
  const T16* wrowB = wgt + (long)(k0 + sb_n) * b_row_stride + sb_c;
  short8 breg[2];
  auto load_b = [&](int tap, int cc) {
    const T16* wp = wrowB + (long)tap * b_rs_stride + cc * BK;
    breg[0] = *reinterpret_cast<const short8*>(wp);
    breg[1] = *reinterpret_cast<const short8*>(wp + 8);
  };
  auto stage_b = [&]() {
    short* pb = reinterpret_cast<short*>(
        ldsB + (ROWST ? epi_brow<2>(sb_n) : sb_n) * LDK + sb_c);
    *reinterpret_cast<short8*>(pb) = breg[0];
    *reinterpret_cast<short8*>(pb + 8) = breg[1];
  };

  load_b(0, 0);

  for (int cc = 0; cc < cchunks; ++cc) {
    __syncthreads();  // previous c-chunk's patch reads done
    // ---- cooperative patch stage: rows gr0..gr0+NR-1, cols -1..Wi.
    // 4-deep load batches: the load->store pairs of the plain loop expose
    // one L2/HBM round trip per group (the fill is this kernel's dominant
    // serial phase — PMC: 67% parked) ----
    const int ngroups = NR * (Wi + 2) * (BK / 8);
    for (int i0f = tid; i0f < ngroups; i0f += 4 * 256) {
      const T16* srcs[4];
      short8 vals[4];
      int dsts[4], gs[4];
      bool ok[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int i = i0f + b * 256;
        const int g = i % (BK / 8);
        const int ce = i / (BK / 8);
        const int col = ce % (Wi + 2);
        const int row = ce / (Wi + 2);
        const long gr = gr0 + row;
        const int iw = col - 1;
        gs[b] = g;
        dsts[b] = i < ngroups ? (row * (Wi + 2) + col) * PCS + g * 8 : -1;
        ok[b] = i < ngroups && gr >= 0 && gr < (long)N * Ho &&
                (unsigned)iw < (unsigned)Wi;
        const long nn = ok[b] ? gr / Ho : 0;
        const long pp = ok[b] ? gr % Ho : 0;
        srcs[b] = ok[b]
                      ? in + ((nn * Hi + pp) * Wi + iw) * CI + cc * BK + g * 8
                      : zstub;  // always-loadable: batches the 4 round trips
      }
#pragma unroll
      for (int b = 0; b < 4; ++b)
        vals[b] = *reinterpret_cast<const short8*>(srcs[b]);
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        if (dsts[b] < 0) break;
        short8 v = vals[b];
        if (!ok[b]) v = short8{};
        if constexpr (SCALED) {
          if (ok[b])
            v = scale8<T16>(v, sc8_load(asc, ash, cc * BK + gs[b] * 8));
        }
        *reinterpret_cast<short8*>(patch + dsts[b]) = v;
      }
    }
    __syncthreads();

#pragma unroll
    for (int r = 0; r < 3; ++r) {
      // tap row validity is per-lane but constant over s and kk
      const int pv = TRANS ? p_lane + 1 - r : p_lane + r - 1;
      const bool rv = m_ok && (unsigned)pv < (unsigned)Ho;
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const int tap = r * 3 + s;
        const long off = TRANS
                             ? ((long)(1 - r) * (Wi + 2) + (1 - s)) * PCS
                             : ((long)(r - 1) * (Wi + 2) + (s - 1)) * PCS;
        const T16* abase = rv ? patch + lane_base + off : zstub;
        __syncthreads();  // previous tap's MFMAs done reading ldsB
        stage_b();
        __syncthreads();
        // next tap's (or next c-chunk's) B burst rides under the MFMAs
        if (tap < 8)
          load_b(tap + 1, cc);
        else if (cc + 1 < cchunks)
          load_b(0, cc + 1);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const short8 af = *reinterpret_cast<const short8*>(
              abase + kk * 16 + kh * 8);
          const short8 b0 = *reinterpret_cast<const short8*>(
              ldsB + li * LDK + kk * 16 + kh * 8);
          const short8 b1 = *reinterpret_cast<const short8*>(
              ldsB + (32 + li) * LDK + kk * 16 + kh * 8);
          acc[0] = Mfma32<T16>::run(af, b0, acc[0]);
          acc[1] = Mfma32<T16>::run(af, b1, acc[1]);
        }
      }
    }
  }

  // ---- epilogue: bias + act (+ optional BN-stats partials) in fp32
  // registers, one rounding, then the store. ch[t2]: the lane's output
  // channel in accumulator tile t2 ----
  const int ch[2] = {ROWST ? 2 * li : li, ROWST ? 2 * li + 1 : 32 + li};
  float bv[2];
  bv[0] = has_bias ? bias[k0 + ch[0]] : 0.f;
  bv[1] = has_bias ? bias[k0 + ch[1]] : 0.f;
  float ssum[2] = {}, ssq[2] = {};
  if constexpr (ROWST) {
    // whole rows, 16 bytes per lane: each wave brings its 32 x 64 addin
    // tile into its own part of the patch LDS (which no tap reads any
    // more), adds in registers, and sends the rounded tile back the same
    // way (conv_epilogue.h)
    using E = EpiTile<2>;
    short* wl = reinterpret_cast<short*>(psmem) + wave * E::WAVE;
    long roff[E::NIT];
#pragma unroll
    for (int it = 0; it < E::NIT; ++it) {
      const long m = bm0 + wm + epi_io_row<2>(it, lane);
      roff[it] = m < Mtot ? m * KO + k0 : -1;
    }
    __syncthreads();  // every wave's last tap is done reading the patch
    if constexpr (ADDIN) {
      epi_fetch<T16, 2>(wl, addin, lane, roff);
      epi_wave_sync();
    }
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int row = epi_acc_row(reg, kh);
      short2v h = {};
      if (bm0 + wm + row < Mtot) {
        if constexpr (ADDIN) h = epi_get<2>(wl, row, li);
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2) {
          float v = acc[t2][reg] + bv[t2];
          if constexpr (ADDIN) v += s16_to_f32<T16>(h[t2]);
          if (act == 1) v = relu_f(v);
          if (stats_slab) {
            ssum[t2] += v;
            ssq[t2] += v * v;
          }
          h[t2] = f32_to_s16<T16>(v);
        }
      }
      epi_put<2>(wl, row, li, h);
    }
    epi_wave_sync();
    epi_flush<T16, 2>(wl, out, lane, roff);
  } else {
    // one 16-bit element per lane straight from the accumulator
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const long m_out = bm0 + wm + epi_acc_row(reg, kh);
      if (m_out < Mtot) {
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2) {
          float v = acc[t2][reg] + bv[t2];
          if (act == 1) v = relu_f(v);
          if (stats_slab) {
            ssum[t2] += v;
            ssq[t2] += v * v;
          }
          out[m_out * KO + k0 + ch[t2]] = F16<T16>::from_f32(v);
        }
      }
    }
  }
  if (stats_slab) {
    // conv->BN fusion (same fold as conv_gather_gemm): kh halves by
    // xor-shuffle, waves by per-wave LDS rows (no LDS atomics)
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {
      ssum[t2] += __shfl_xor(ssum[t2], 32, 64);
      ssq[t2] += __shfl_xor(ssq[t2], 32, 64);
    }
    float* lsum = reinterpret_cast<float*>(psmem);  // [4 waves][128]
    __syncthreads();  // patch reads / staged-tile read-back (same LDS) done
    if (kh == 0) {
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2) {
        lsum[wave * 128 + ch[t2]] = ssum[t2];
        lsum[wave * 128 + 64 + ch[t2]] = ssq[t2];
      }
    }
    __syncthreads();
    float* slab =
        stats_slab + ((long)blockIdx.y * gridDim.x + blockIdx.x) * 2 * 64;
    for (int t = tid; t < 2 * 64; t += 256)
      slab[t] = lsum[t] + lsum[128 + t] + lsum[256 + t] + lsum[384 + t];
  }
}

// ---------------------------------------------------------------------------
// Ring variant of the patch kernel for the 64-channel 3x3/s1 layer
// (CI == 64, W == 32, H % 4 == 0; fwd, dgrad, dgrad + ADDIN). At CI == 64
// conv_patch_gemm's block lives for one patch fill and nine short taps, each
// with its own weight stage and two barriers, and every 4-row tile fetches 6
// input rows. Here a block stays on its CU and walks whole images
// (blockIdx.x, + gridDim.x, ...) in steps of 128 outputs = 4 image rows:
//   weights: the block's 64 x 576 tile is read ONCE, straight into registers
//   (36 x 16 B per lane: the lane's own MFMA B fragments for all nine taps),
//   so the loop has no weight stage, no weight LDS reads and no barriers for
//   them.
//   input: a ring of 12 image rows ([34][PCS] each, pad columns zeroed once).
//   A step reads rows 4t-1 .. 4t+4 and only ever fetches 4 new ones: the
//   16 KB of step t+2 are on their way into registers during all of step
//   t-1 and step t's taps, and are written after those taps to the slot
//   step t-1 owned. Rows outside the image are not staged; their taps read
//   the zero stub, as in conv_patch_gemm.
//   waves: 8, as 4 (image rows of the step) x 2 (halves of the 64 output
//   channels), one 32x32 accumulator each; per output element the MFMAs are
//   the same instruction in the same order (tap 0..8, kk 0..3) as in
//   conv_patch_gemm, so results are bit-identical.
//   epilogue: the two waves of a row share a [32][RS] staging tile (even
//   channels from one, odd from the other) and store whole 128-byte rows;
//   ADDIN reads its tile the same way. The 2-byte store straight from the
//   accumulator needs 256 VGPRs and spills here, so no variant uses it.
//   stats: one 128-float slab row per 128-output TILE, folded in
//   conv_patch_gemm's order (registers, kh halves, then the 4 row waves).
// Two block barriers per step.
// ---------------------------------------------------------------------------
constexpr int RG_W = 32;                        // image width
constexpr int RG_ROW = (RG_W + 2) * PCS;        // elements of one ring row
constexpr int RG_SLOTS = 3;                     // 4-row slots in the ring
constexpr int RG_ES = EpiTile<2>::RS;           // staged output row stride
constexpr int RG_LDS = (RG_SLOTS * 4 * RG_ROW + PCS + 4 * 32 * RG_ES) * 2 +
                       4 * 128 * 4;             // bytes

template <typename T16, bool TRANS, bool ADDIN>
__global__ __launch_bounds__(512) void conv_patch_ring(
    const T16* __restrict__ in,   // [N, Hi, 32, 64] (dgrad: dy)
    const T16* __restrict__ wgt,  // fwd: [KO, 9*64]; dgrad: wflip strides
    const float* __restrict__ bias,
    const T16* __restrict__ addin,  // ADDIN only: out += addin
    T16* __restrict__ out,          // [N, Hi, 32, KO]
    float* __restrict__ stats_slab,  // null, or per-tile (sum,sumsq) rows
    const int N, const int Hi, const int KO, const long b_row_stride,
    const long b_rs_stride, const int act, const int has_bias) {
  __shared__ __attribute__((aligned(16))) char rsmem[RG_LDS];
  T16* ring = reinterpret_cast<T16*>(rsmem);  // [12 rows][34][PCS]
  T16* zstub = ring + RG_SLOTS * 4 * RG_ROW;  // 72 zero elements
  short* stage = reinterpret_cast<short*>(zstub + PCS);  // [4][32][RG_ES]
  float* lsum = reinterpret_cast<float*>(stage + 4 * 32 * RG_ES);  // [4][128]

  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int li = lane & 31;  // output column (A row) and channel (B row)
  const int kh = lane >> 5;
  const int wr = wave >> 1;  // the step's image row this wave computes
  const int wk = wave & 1;   // its half of the 64 output channels
  const int k0 = blockIdx.y * 64;
  const int G = gridDim.x;
  const int TPI = Hi >> 2;  // steps (128-output tiles) per image
  const int nsteps = ((N - (int)blockIdx.x + G - 1) / G) * TPI;

  // zero stub and the pad columns (0 and 33) of every ring row, once: the
  // fill only ever writes columns 1..32
  if (tid < 64) zstub[tid] = T16{};
  if (tid < RG_SLOTS * 4 * 2 * 8) {
    const int row = tid >> 4, side = (tid >> 3) & 1, g8 = tid & 7;
    *reinterpret_cast<short8*>(ring + row * RG_ROW +
                               side * (RG_W + 1) * PCS + g8 * 8) = short8{};
  }

  // the lane's output channel within the k-tile, and its B fragments
  const int ch = 2 * li + wk;
  short8 bf[9][4];
  {
    const T16* wp = wgt + (long)(k0 + ch) * b_row_stride + kh * 8;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
        bf[tap][kk] = *reinterpret_cast<const short8*>(
            wp + tap * b_rs_stride + kk * 16);
  }
  const float bv = has_bias ? bias[k0 + ch] : 0.f;

  // fill: a 4-row group is 16 KB contiguous in global memory; thread `tid`
  // moves 16-byte pieces tid and tid + 512 (rows tid/256 and tid/256 + 2)
  const int f_dst =
      ((tid >> 8) * (RG_W + 2) + ((tid >> 3) & 31) + 1) * PCS + (tid & 7) * 8;
  auto group_load = [&](int n, int g, short8(&v)[2]) {
    const T16* src = in + ((long)n * Hi + 4 * g) * (RG_W * 64) + tid * 8;
    v[0] = *reinterpret_cast<const short8*>(src);
    v[1] = *reinterpret_cast<const short8*>(src + 512 * 8);
  };
  auto ring_put = [&](int slot, const short8(&v)[2]) {
    T16* d = ring + slot * 4 * RG_ROW + f_dst;
    *reinterpret_cast<short8*>(d) = v[0];
    *reinterpret_cast<short8*>(d + 2 * RG_ROW) = v[1];
  };

  // (image, group) of the block's flat step sequence, advanced by one
  auto advance = [&](int& n, int& g) {
    if (++g == TPI) {
      g = 0;
      n += G;
    }
  };
  // Prefetch: pv holds the group of step it+2 while step it runs; it is
  // fetched as soon as the group before it has left the registers for the
  // ring, a whole step earlier. A fetch past the block's last group repeats
  // that group (and its put lands in a slot no step reads any more), so the
  // loop body has no branch around a load and the compiler can count the
  // loads in flight instead of waiting for all. Two or three register sets
  // (groups fetched two or three steps ahead) measured the same.
  int pn = blockIdx.x, pg = 0, pleft = nsteps - 1;  // next group to fetch
  auto fetch = [&](short8(&v)[2]) {
    group_load(pn, pg, v);
    if (pleft > 0) {
      --pleft;
      advance(pn, pg);
    }
  };
  short8 pv[2];
  for (int fg = 0; fg < 2; ++fg) {
    fetch(pv);
    ring_put(fg, pv);
  }
  fetch(pv);

  // output rows this lane moves in the row store: the pair's tile is
  // 32 rows x 128 B, each wave takes 16 rows, 8 lanes per row
  const int io_row = wk * 16 + (lane >> 3);
  const int io_c = (lane & 7) * 8;
  short* st = stage + wr * 32 * RG_ES;
  auto out_off = [&](long tile, int b) {
    return (tile * 128 + wr * 32 + io_row + b * 8) * KO + k0 + io_c;
  };
  short8 av[2];  // ADDIN: the lane's pieces of the step's addin tile
  if constexpr (ADDIN) {
#pragma unroll
    for (int b = 0; b < 2; ++b)
      av[b] = *reinterpret_cast<const short8*>(
          addin + out_off((long)blockIdx.x * TPI, b));
  }

  // The weight loads must have landed before the loop, not in it: a use
  // here makes the compiler wait for them now. Otherwise it has to assume
  // they may still be in flight at the loop's first MFMA and waits there,
  // in every step, for everything in flight.
#pragma unroll
  for (int tap = 0; tap < 9; ++tap)
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) asm volatile("" : "+v"(bf[tap][kk]));
  __syncthreads();

  int n_img = blockIdx.x, g = 0, slot = 0;  // slot = step % 3
  for (int it = 0; it < nsteps; ++it) {
    const long tile = (long)n_img * TPI + g;
    int n2 = n_img, g2 = g;  // the next step's tile (the last: itself)
    if (it + 1 < nsteps) advance(n2, g2);

    f32x16 acc = {};
    const int prow = 4 * g + wr;
    // the tap's A fragments (4 x 16 B per lane). Its source row is
    // wave-uniform; outside the image -> zero stub
    auto a_load = [&](int tap, short8(&af)[4]) {
      const int r = tap / 3, s = tap % 3;
      const int dr = TRANS ? 1 - r : r - 1;
      const int dc = TRANS ? 1 - s : s - 1;
      const bool rv = (unsigned)(prow + dr) < (unsigned)Hi;
      int rr = slot * 4 + wr + dr;
      rr += rr < 0 ? RG_SLOTS * 4 : 0;
      rr -= rr >= RG_SLOTS * 4 ? RG_SLOTS * 4 : 0;
      const T16* abase =
          (rv ? ring + rr * RG_ROW + (li + 1 + dc) * PCS : zstub) + kh * 8;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
        af[kk] = *reinterpret_cast<const short8*>(abase + kk * 16);
    };
    // one tap ahead: the next tap's four reads are in flight under this
    // tap's MFMAs (3 % faster than reading each tap where it is used)
    short8 af[2][4];
    a_load(0, af[0]);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      if (tap < 8) a_load(tap + 1, af[(tap + 1) & 1]);
      // keep the reads up here: the scheduler otherwise sinks them to just
      // before this tap's last MFMA
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
        acc = Mfma32<T16>::run(af[tap & 1][kk], bf[tap][kk], acc);
    }

    // ---- epilogue: bias + act (+ ADDIN, + stats partials) in fp32
    // registers, one rounding, as in conv_patch_gemm ----
    float ssum = 0.f, ssq = 0.f;
    if constexpr (ADDIN) {
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        *reinterpret_cast<short8*>(st + (io_row + b * 8) * RG_ES + io_c) =
            av[b];
        // the next step's tile is on its way from here on
        av[b] = *reinterpret_cast<const short8*>(
            addin + out_off((long)n2 * TPI + g2, b));
      }
    }
    // every wave is done with this step's ring rows and with the staging
    // tile of the previous step; the pair's addin tile is in place
    __syncthreads();
    ring_put(slot == 0 ? 2 : slot - 1, pv);  // group it+2
    fetch(pv);                               // group it+3
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      short* e = st + epi_acc_row(reg, kh) * RG_ES + ch;
      float v = acc[reg] + bv;
      if constexpr (ADDIN) v += s16_to_f32<T16>(*e);
      if (act == 1) v = relu_f(v);
      if (stats_slab) {
        // conv_patch_gemm's chain, row by row: its rows are separate
        // branches, so its v * v is fused into the running sum one row
        // at a time. Spelled out here, where the straight-line loop
        // would let the compiler fuse the products in another order.
        ssum += v;
        ssq = __builtin_fmaf(v, v, ssq);
      }
      *e = f32_to_s16<T16>(v);
    }
    if (stats_slab) {
      ssum += __shfl_xor(ssum, 32, 64);
      ssq += __shfl_xor(ssq, 32, 64);
      if (kh == 0) {
        lsum[wr * 128 + ch] = ssum;
        lsum[wr * 128 + 64 + ch] = ssq;
      }
    }
    __syncthreads();  // new ring rows, staged tile and stats rows visible
#pragma unroll
    for (int b = 0; b < 2; ++b)
      *reinterpret_cast<short8*>(out + out_off(tile, b)) =
          *reinterpret_cast<const short8*>(st + (io_row + b * 8) * RG_ES +
                                           io_c);
    if (stats_slab && tid < 128) {
      float* slab =
          stats_slab + ((long)blockIdx.y * ((long)N * TPI) + tile) * 128;
      slab[tid] =
          lsum[tid] + lsum[128 + tid] + lsum[256 + tid] + lsum[384 + tid];
    }
    n_img = n2;
    g = g2;
    slot = slot == 2 ? 0 : slot + 1;
  }
}

// ---------------------------------------------------------------------------
// Streaming variant of the patch kernel for the 128/256/512-channel 3x3/s1
// layers (CI % 64 == 0, CI >= 128, W in {4, 8, 16}; fwd, dgrad, dgrad +
// ADDIN). conv_patch_gemm's block lives for CI/64 c-chunks; each is a patch
// fill behind a barrier and nine weight-tile stages behind two barriers each
// (20 barriers for 72 MFMAs per wave), and every 128-output block re-stages
// the k-tile's weights. Here one 512-thread block per CU keeps one 64-channel
// output tile (k-tile) and walks m-tiles of 256 outputs (its rank, + blocks
// of that k-tile, ...) as ONE flat sequence of stages (m-tile, c-chunk):
//   operands of a stage: the input patch of the 256 outputs ([256/W + 2
//   rows][W + 2][PCS], pad columns zeroed once) and the whole 64 x 9 x 64
//   weight slice ([9][64][LDK]). Those of stage i+1 are requested (14
//   global_load_dwordx4 per thread, into registers) right after stage i's
//   operands are in LDS, travel during its 72 MFMAs per wave, and are written
//   to LDS between the two barriers that separate the stages. Whether i+1 is
//   the next c-chunk or the next m-tile makes no difference. The fetch after
//   the block's last stage repeats it and is never written.
//   waves: 2 groups x 4; a group owns a 128-output half, a wave 32 m x 64 k
//   as two 32x32 accumulators: conv_patch_gemm's wave tile, and per output
//   element the same MFMAs in the same order (c-chunk, tap 0..8, kk 0..3),
//   so results are bit-identical.
//   epilogue: runs after the NEXT stage's operands are in LDS and the stage
//   after that is requested, so its stores are not waited for until a whole
//   stage later. Each wave stages 16 rows at a time in a private tile and
//   stores whole 128-byte rows (conv_epilogue.h); the ADDIN tile is requested
//   a stage ahead and arrives through the same tile.
//   stats: one 128-float slab row per 128-output half, folded in
//   conv_patch_gemm's order (registers, kh halves, the group's 4 waves).
// Two block barriers per stage. W divides 256, so every tile starts at the
// beginning of an image row; vertical pad, image changes inside a tile and
// the M tail are a per-lane address select onto the zero stub. Patch rows
// outside the tensor hold a clamped (valid) address's data; no lane with a
// valid output reads them.
// LDS (bytes): weights 82,944 + stub 144 + staging 8 x 2,304 = 18,432 + stats
// rows 4,096 = 105,616, + patch 46,656 (W = 16), 48,960 (W = 8) or 57,024
// (W = 4): 152,272 / 154,576 / 162,640 of 163,840. Declared for W = 4.
// ---------------------------------------------------------------------------
constexpr int ST_M = 256;                              // outputs per m-tile
constexpr int ST_WIMG = 9 * 64 * LDK;                  // weight image, elements
constexpr int ST_PATCH = (ST_M / 4 + 2) * (4 + 2) * PCS;  // W = 4: the largest
constexpr int ST_EPI = EpiTile<2, 16>::WAVE;           // a wave's staging tile
constexpr int ST_LDS =
    (ST_PATCH + PCS + ST_WIMG + 8 * ST_EPI) * 2 + 8 * 128 * 4;  // bytes
static_assert(ST_LDS <= 160 * 1024, "conv_patch_stream: LDS over 160 KiB");

template <typename T16, bool TRANS, bool ADDIN>
__global__ __launch_bounds__(512) void conv_patch_stream(
    const T16* __restrict__ in,   // [N, Hi, W, CI] (dgrad: dy)
    const T16* __restrict__ wgt,  // fwd: [KO, 9*CI]; dgrad: wflip strides
    const float* __restrict__ bias,
    const T16* __restrict__ addin,  // ADDIN only: out += addin
    T16* __restrict__ out,          // [N, Hi, W, KO]
    float* __restrict__ stats_slab,  // null, or per-half (sum,sumsq) rows
    const int N, const int Hi, const int lw /* log2 W */, const int CI,
    const int KO, const long b_row_stride, const long b_rs_stride,
    const int act, const int has_bias, const int xcd_local) {
  using E = EpiTile<2, 16>;
  __shared__ __attribute__((aligned(16))) char ssmem[ST_LDS];
  const int W = 1 << lw;
  T16* wimg = reinterpret_cast<T16*>(ssmem);  // [9][64][LDK]
  T16* zstub = wimg + ST_WIMG;                // 72 zero elements
  short* stage = reinterpret_cast<short*>(zstub + PCS);  // [8][16][E::RS]
  float* lsum = reinterpret_cast<float*>(stage + 8 * ST_EPI);  // [8][128]
  T16* patch = reinterpret_cast<T16*>(lsum + 8 * 128);

  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int li = lane & 31;
  const int kh = lane >> 5;
  const int wm = wave * 32;  // the wave's m-rows within the tile

  // k-tile and rank of this block among the blocks of its k-tile. Blocks b
  // and b + 8 share an XCD: with xcd_local the blocks of a k-tile sit on as
  // few XCDs as possible, so its weights stay in their L2s (speed only).
  const int KT = KO / 64;
  const int cnt = gridDim.x / KT;  // the host makes the grid a multiple
  int ky, rank;
  if (xcd_local) {
    ky = ((int)blockIdx.x & 7) % KT;
    rank = ((int)blockIdx.x >> 3) * (8 / KT) + ((int)blockIdx.x & 7) / KT;
  } else {
    ky = (int)blockIdx.x % KT;
    rank = (int)blockIdx.x / KT;
  }
  const int k0 = ky * 64;
  const long Mtot = (long)N * Hi * W;
  const int MT = (int)((Mtot + ST_M - 1) / ST_M);
  const int cchunks = CI / BK;
  const int ntiles = rank < MT ? (MT - rank + cnt - 1) / cnt : 0;
  const int nstages = ntiles * cchunks;
  if (nstages == 0) return;

  // zero stub and the pad columns (0 and W + 1) of every patch row, once:
  // the fill only ever writes columns 1..W
  const int NR = (ST_M >> lw) + 2;
  if (tid < 64) zstub[tid] = T16{};
  for (int i = tid; i < NR * 16; i += 512) {
    const int row = i >> 4, side = (i >> 3) & 1, g8 = i & 7;
    *reinterpret_cast<short8*>(patch + (row * (W + 2) + side * (W + 1)) * PCS +
                               g8 * 8) = short8{};
  }

  // ---- operand fetch: thread `tid` moves, per tap, the 16-byte piece
  // (weight row tid/8, channels (tid%8)*8..) and five pieces of the patch
  // (pixel tid/8 + 64 b of the tile's NR * W, same channels) ----
  const int f_n = tid >> 3, f_c = (tid & 7) * 8;
  const T16* wsrc = wgt + (long)(k0 + f_n) * b_row_stride + f_c;
  const int w_dst = epi_brow<2>(f_n) * LDK + f_c;
  const int p_dst = ((f_n >> lw) * (W + 2) + (f_n & (W - 1)) + 1) * PCS + f_c;
  const int p_step = (64 >> lw) * (W + 2) * PCS;  // 64 pixels further
  const bool p_tail = f_n < 2 * W;  // piece 4 exists (NR * W = 256 + 2 W)
  short8 wv[9], pv[5];
  auto fetch = [&](long m0, int cc) {
    const T16* wp = wsrc + cc * BK;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
      wv[tap] = *reinterpret_cast<const short8*>(wp + tap * b_rs_stride);
    const T16* ip = in + cc * BK + f_c;
#pragma unroll
    for (int b = 0; b < 5; ++b) {
      // pixel of the tensor, clamped into it: always loadable
      long px = m0 - W + f_n + 64 * b;
      px = px < 0 ? 0 : px;
      px = px < Mtot ? px : Mtot - 1;
      pv[b] = *reinterpret_cast<const short8*>(ip + px * CI);
    }
  };
  auto put = [&]() {
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
      *reinterpret_cast<short8*>(wimg + tap * 64 * LDK + w_dst) = wv[tap];
#pragma unroll
    for (int b = 0; b < 4; ++b)
      *reinterpret_cast<short8*>(patch + p_dst + b * p_step) = pv[b];
    if (p_tail) *reinterpret_cast<short8*>(patch + p_dst + 4 * p_step) = pv[4];
  };
  // the block's flat stage sequence; the fetch past its end repeats the
  // last stage, so no load sits behind a branch
  int f_t = rank, f_cc = 0, f_left = nstages - 1;
  auto fetch_next = [&]() {
    fetch((long)f_t * ST_M, f_cc);
    if (f_left > 0) {
      --f_left;
      if (++f_cc == cchunks) {
        f_cc = 0;
        f_t += cnt;
      }
    }
  };

  // ---- per-lane A coordinates: fixed within the tile, since every tile
  // starts at the beginning of an image row ----
  const int prow = ((wm + li) >> lw) + 1;
  const int pcol = ((wm + li) & (W - 1)) + 1;
  const T16* a_lane = patch + (prow * (W + 2) + pcol) * PCS + kh * 8;
  const T16* a_zero = zstub + kh * 8;
  const T16* b_lane = wimg + li * LDK + kh * 8;

  // ---- epilogue of one m-tile: bias + act (+ ADDIN, + stats partials) in
  // fp32 registers, one rounding, as in conv_patch_gemm ----
  const int ch0 = 2 * li;  // the lane's channels: ch0 (acc[0]), ch0 + 1
  float bv[2];
  bv[0] = has_bias ? bias[k0 + ch0] : 0.f;
  bv[1] = has_bias ? bias[k0 + ch0 + 1] : 0.f;
  short* wl = stage + wave * ST_EPI;
  const int io_row = lane >> 3, io_c = (lane & 7) * 8;
  short8 av[2][E::NIT];  // ADDIN: the lane's pieces of the tile's addin rows
  auto addin_load = [&](long m0) {
#pragma unroll
    for (int half = 0; half < 2; ++half)
#pragma unroll
      for (int it = 0; it < E::NIT; ++it) {
        long m = m0 + wm + half * 16 + it * E::RPI + io_row;
        m = m < Mtot ? m : Mtot - 1;  // rows past the end are never used
        av[half][it] =
            *reinterpret_cast<const short8*>(addin + m * KO + k0 + io_c);
      }
  };
  f32x16 acc[2] = {};
  auto epilogue = [&](long m0) {
    const long bm = m0 + wm;
    float ssum[2] = {}, ssq[2] = {};
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      long roff[E::NIT];
#pragma unroll
      for (int it = 0; it < E::NIT; ++it) {
        const long m = bm + half * 16 + epi_io_row<2>(it, lane);
        roff[it] = m < Mtot ? m * KO + k0 : -1;
      }
      epi_wave_sync();  // the wave's previous pass has been read back
      if constexpr (ADDIN) {
#pragma unroll
        for (int it = 0; it < E::NIT; ++it)
          *reinterpret_cast<short8*>(wl + epi_io_row<2>(it, lane) * E::RS +
                                     io_c) = av[half][it];
        epi_wave_sync();
      }
#pragma unroll
      for (int r8 = 0; r8 < 8; ++r8) {
        const int reg = half * 8 + r8;
        const int row = epi_acc_row(reg, kh);
        short2v h = {};
        if (bm + row < Mtot) {
          if constexpr (ADDIN) h = epi_get<2>(wl, row - half * 16, li);
#pragma unroll
          for (int t2 = 0; t2 < 2; ++t2) {
            float v = acc[t2][reg] + bv[t2];
            if constexpr (ADDIN) v += s16_to_f32<T16>(h[t2]);
            if (act == 1) v = relu_f(v);
            if (stats_slab) {
              // conv_patch_gemm's chain: v * v fused into the running sum
              // row by row (see conv_patch_ring)
              ssum[t2] += v;
              ssq[t2] = __builtin_fmaf(v, v, ssq[t2]);
            }
            h[t2] = f32_to_s16<T16>(v);
          }
        }
        epi_put<2>(wl, row - half * 16, li, h);
      }
      epi_wave_sync();
      epi_flush<T16, 2, 16>(wl, out, lane, roff);
    }
    if (stats_slab) {
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2) {
        ssum[t2] += __shfl_xor(ssum[t2], 32, 64);
        ssq[t2] += __shfl_xor(ssq[t2], 32, 64);
      }
      if (kh == 0) {
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2) {
          lsum[wave * 128 + ch0 + t2] = ssum[t2];
          lsum[wave * 128 + 64 + ch0 + t2] = ssq[t2];
        }
      }
    }
  };
  // the slab rows of a tile whose epilogue every wave has finished (a block
  // barrier lies between): one row per 128-output half that exists
  const long nt128 = (Mtot + 127) / 128;
  auto slab_write = [&](long tile) {
    if (tid < 256) {
      const int g2 = tid >> 7, t = tid & 127;
      const long row = tile * 2 + g2;
      const float* l = lsum + g2 * 4 * 128 + t;
      if (row < nt128)
        stats_slab[((long)ky * nt128 + row) * 128 + t] =
            l[0] + l[128] + l[256] + l[384];
    }
  };

  fetch_next();  // stage 0

  int tile = rank, cc = 0;
  long e_tile = -1;  // the tile whose epilogue is still to run
  bool s_pend = false;  // lsum holds e_tile's partials, slab not written
  long s_tile = 0;
  for (int s = 0; s < nstages; ++s) {
    const long m0 = (long)tile * ST_M;
    __syncthreads();  // every wave is done with the previous stage's LDS
    put();
    if (stats_slab && s_pend) {
      slab_write(s_tile);
      s_pend = false;
    }
    __syncthreads();  // operands (and, at s == 0, the zeroed pads) visible
    fetch_next();  // stage s + 1
    if (e_tile >= 0) {
      epilogue(e_tile * ST_M);
      if (stats_slab) {
        s_pend = true;
        s_tile = e_tile;
      }
      e_tile = -1;
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) acc[t2][reg] = 0.f;
    }
    if constexpr (ADDIN) {
      // this tile's addin rows, for the epilogue a stage from now
      if (cc == cchunks - 1) addin_load(m0);
    }

    // tap-row validity is per lane, constant over s and kk
    const long m_lane = m0 + wm + li;
    const int p_lane = (int)((m_lane >> lw) % Hi);
    const bool m_ok = m_lane < Mtot;
    // One flat sequence of 36 steps (tap, kk), each one A and two B
    // fragments and two MFMAs. The reads of step i + 2 are issued before the
    // MFMAs of step i (three fragment sets), so an MFMA never waits for a
    // read the wave has just issued; the scheduling barriers keep the
    // compiler from moving the reads back to their use.
    struct Frag {
      short8 a, b0, b1;
    };
    constexpr int PD = 2;  // steps ahead
    Frag fr[PD + 1];
    auto frag_load = [&](int st, Frag& f) {
      const int tap = st >> 2, kk = st & 3;
      const int r = tap / 3, sx = tap % 3;
      const int dr = TRANS ? 1 - r : r - 1;
      const int dc = TRANS ? 1 - sx : sx - 1;
      const bool rv = m_ok && (unsigned)(p_lane + dr) < (unsigned)Hi;
      const T16* abase = rv ? a_lane + (dr * (W + 2) + dc) * PCS : a_zero;
      const T16* bt = b_lane + tap * 64 * LDK + kk * 16;
      f.a = *reinterpret_cast<const short8*>(abase + kk * 16);
      f.b0 = *reinterpret_cast<const short8*>(bt);
      f.b1 = *reinterpret_cast<const short8*>(bt + 32 * LDK);
    };
#pragma unroll
    for (int st = 0; st < PD; ++st) frag_load(st, fr[st]);
#pragma unroll
    for (int st = 0; st < 36; ++st) {
      if (st + PD < 36) frag_load(st + PD, fr[(st + PD) % (PD + 1)]);
      __builtin_amdgcn_sched_barrier(0);
      const Frag& f = fr[st % (PD + 1)];
      acc[0] = Mfma32<T16>::run(f.a, f.b0, acc[0]);
      acc[1] = Mfma32<T16>::run(f.a, f.b1, acc[1]);
      __builtin_amdgcn_sched_barrier(0);
    }

    if (++cc == cchunks) {
      cc = 0;
      e_tile = tile;
      tile += cnt;
    }
  }
  // the last tile. With one c-chunk per tile the tile before it still has
  // its partials in lsum here (block-uniform condition)
  if (stats_slab && s_pend) {
    __syncthreads();
    slab_write(s_tile);
    __syncthreads();
  }
  epilogue(e_tile * ST_M);
  if (stats_slab) {
    __syncthreads();
    slab_write(e_tile);
  }
}

// wgrad: dw[KO, kg] = sum_m dy[m, KO] * A_im2col[m, kg]. MFMA reduces over
// its register-minor k dim, which here is m — both operands are m-major in
// memory, so both tiles are staged TRANSPOSED into LDS ([k][m] / [kg][m]),
// packing 4 m-values per ds_write_b64 during staging. Each block owns a
// 64(KO) x 64(kg at one (r,s,c-chunk)) output tile and an m-chunk; each
// chunk stores a disjoint fp32 partial slab (split-M fills the chip for
// the small late-layer filter counts) and wgrad_reduce_chunks sums them —
// fp32 atomicAdd on the small dw region measured ~21 ns/op amortized.
// ---------------------------------------------------------------------------

namespace {

constexpr int WGM = 64;   // m per step
constexpr int LDM = 72;   // m-minor row length (+16B: alignment + banks)

// KT = KO-tile width (64 or 128): wider k-tiles amortize the x staging
// and double the MFMA work per m-step for the K>=128 layers.
template <typename T16, int KT, bool SCALED = false, bool KMIN = false>
// the second launch-bounds arg (min 2 blocks/CU) is load-bearing: without
// it the compiler allocates 188-256 VGPRs (occupancy 1-2) for no speedup;
// with it 104-124 VGPRs, zero spills, occupancy 4 - the extra waves are
// what covers the gather's HBM latency (PMC: 66% WAIT_ANY at occ 2).
// SCALED variants pin the unscaled occupancy (the Sc8 regs cost a tier).
// KMIN: k-minor staging + rotate-swizzled columns (conv_wgrad_mfma_s3).
__global__ __launch_bounds__(256, SCALED ? 4 : 2) void conv_wgrad_mfma_kernel(
    const T16* __restrict__ x,    // [N, Hi, Wi, CI]
    const T16* __restrict__ dy,   // [M, KO]
    const float* __restrict__ asc,  // SCALED only: [CI] lazy-BN scale
    const float* __restrict__ ash,
    float* __restrict__ dw,       // [KO, R*S*CI]
    const int N, const int Hi, const int Wi, const int CI, const int KO,
    const int Ho, const int Wo, const int R, const int S, const int stride,
    const int pad, const long m_per_chunk, const int nchunks) {
  __shared__ T16 lds[(KT + 64) * LDM];

  const int tid = threadIdx.x;
  const long Mtot = (long)N * Ho * Wo;
  const int k0 = blockIdx.x * KT;
  const int cchunks = CI / BK;
  const int c0 = (blockIdx.y % cchunks) * BK;
  const int s_ = (blockIdx.y / cchunks) % S;
  const int r_ = blockIdx.y / (cchunks * S);
  const long m_begin = (long)blockIdx.z * m_per_chunk;
  const long m_end = min(Mtot, m_begin + m_per_chunk);

  // staging: dyT uses 2*KT threads (4 m-rows x 8 k each); xT uses 128
  // threads — the upper half when KT==64 (disjoint roles), the lower half
  // when KT==128 (sequential double duty)
  const bool do_dy = tid < 2 * KT;
  const bool do_x = KT == 64 ? tid >= 128 : tid < 128;
  const int t = do_dy ? tid : 0;
  constexpr int KG = KT / 8;             // k-groups per operand row set
  const int sm = KMIN ? (t / KG) * 4 : (t & 15) * 4;   // m offset (4 rows)
  const int sk = KMIN ? (t % KG) * 8 : (t >> 4) * 8;   // k offset (dyT rows)
  const int tx = tid & 127;
  const int smx = KMIN ? (tx >> 3) * 4 : (tx & 15) * 4;
  const int skx = KMIN ? (tx & 7) * 8 : (tx >> 4) * 8;

  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int li = lane & 31;
  const int kh = lane >> 5;
  constexpr int NJ = KT / 64;       // kg sub-tiles per wave
  const int i0 = KT == 64 ? (wave & 1) * 32 : wave * 32;  // KO sub-tile
  const int j0base = KT == 64 ? (wave >> 1) * 32 : 0;

  f32x16 acc[NJ] = {};
  Sc8 wsc{};  // SCALED: this thread's x channels are fixed (c0+skx)
  if constexpr (SCALED) {
    if (do_x) wsc = sc8_load(asc, ash, c0 + skx);
  }

  // incremental (n,p,q) decode for the x-gather: one div/mod at entry,
  // add-with-carry as m advances by WGM per step (divisions in the inner
  // loop were ~40% of this kernel's time)
  int dn = 0, dp = 0, dq = 0;
  {
    const long m_first = m_begin + smx;
    dn = (int)(m_first / ((long)Ho * Wo));
    const int pq = (int)(m_first % ((long)Ho * Wo));
    dp = pq / Wo;
    dq = pq % Wo;
  }
  auto advance = [&](int by) {
    dq += by;
    while (dq >= Wo) {
      dq -= Wo;
      if (++dp == Ho) {
        dp = 0;
        ++dn;
      }
    }
  };

  // gather + pack 4 m-rows of 8 elems into registers for m-step m0
  short8 vdy[4], vx[4];
  auto load_m = [&](long m0) {
    if (do_dy) {
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
        const long m = m0 + sm + mi;
        vdy[mi] = m < m_end ? *reinterpret_cast<const short8*>(
                                  dy + m * KO + k0 + sk)
                            : short8{};
      }
    }
    if (do_x) {
      int n_ = dn, p_ = dp, q_ = dq;
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
        const long m = m0 + smx + mi;
        const int ih = p_ * stride - pad + r_;
        const int iw = q_ * stride - pad + s_;
        const bool ok = m < m_end && (unsigned)ih < (unsigned)Hi &&
                        (unsigned)iw < (unsigned)Wi;
        vx[mi] = ok ? *reinterpret_cast<const short8*>(
                          x + (((long)n_ * Hi + ih) * Wi + iw) * CI + c0 +
                          skx)
                    : short8{};
        if constexpr (SCALED) {
          if (ok) vx[mi] = scale8<T16>(vx[mi], wsc);
        }
        if (mi < 3 && ++q_ == Wo) {
          q_ = 0;
          if (++p_ == Ho) {
            p_ = 0;
            ++n_;
          }
        }
      }
      advance(WGM);  // position for the NEXT m-step's gather
    }
  };
  // transpose-write the 4x8 register patches
  auto stage_m = [&]() {
    if (do_dy) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        short4v pk = {vdy[0][e], vdy[1][e], vdy[2][e], vdy[3][e]};
        const int col = KMIN ? ((sm + ((sk + e) & 56)) & 63) : sm;
        *reinterpret_cast<short4v*>(
            reinterpret_cast<short*>(lds + (sk + e) * LDM + col)) = pk;
      }
    }
    if (do_x) {
      T16* ldsT = lds + KT * LDM;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        short4v pk = {vx[0][e], vx[1][e], vx[2][e], vx[3][e]};
        const int col = KMIN ? ((smx + ((skx + e) & 56)) & 63) : smx;
        *reinterpret_cast<short4v*>(
            reinterpret_cast<short*>(ldsT + (skx + e) * LDM + col)) = pk;
      }
    }
  };

  load_m(m_begin);
  for (long m0 = m_begin; m0 < m_end; m0 += WGM) {
    __syncthreads();
    stage_m();
    __syncthreads();
    if (m0 + WGM < m_end) load_m(m0 + WGM);
    const T16* ldsDyT = lds;
    const T16* ldsXT = lds + KT * LDM;
    const int arow = i0 + li;
    const int arot = KMIN ? (arow & 56) : 0;
#pragma unroll
    for (int kk = 0; kk < WGM; kk += 16) {
      const short8 af = *reinterpret_cast<const short8*>(
          ldsDyT + arow * LDM + ((kk + kh * 8 + arot) & 63));
#pragma unroll
      for (int jj = 0; jj < NJ; ++jj) {
        const int brow = j0base + jj * 32 + li;
        const short8 bf = *reinterpret_cast<const short8*>(
            ldsXT + brow * LDM +
            ((kk + kh * 8 + (KMIN ? (brow & 56) : 0)) & 63));
        acc[jj] = Mfma32<T16>::run(af, bf, acc[jj]);
      }
    }
  }

  // ---- scatter the 32x32 fp32 tile, directly in the parameter layout
  // [KO, CI, R, S]. Split-M chunks write DISJOINT per-chunk slabs (plain
  // stores; a reduce kernel sums them) — fp32 atomicAdd contention on the
  // small dw region measured ~21 ns/op amortized (layer1 chunk ablation),
  // dominating the kernel at high chunk counts ----
  const int rs = r_ * S + s_;
  const long RS = (long)R * S;
  float* slab = dw + (long)blockIdx.z * ((long)KO * CI * RS);
#pragma unroll
  for (int jj = 0; jj < NJ; ++jj) {
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int i = (reg & 3) + 8 * (reg >> 2) + 4 * kh;  // KO row
      const int c_abs = c0 + j0base + jj * 32 + li;
      slab[((long)(k0 + i0 + i) * CI + c_abs) * RS + rs] = acc[jj][reg];
    }
  }
}

// 128x128-output-tile wgrad for KO%128 && CI%128 (the ResNet-50 1x1
// bottleneck convs carry ~45% of its FLOPs and can't use the s-grouped
// kernel): each wave owns FOUR 32x32 acc tiles (2 KO x 2 CI), so one
// dy+x stage feeds 16 MFMAs per wave per m-step instead of 8, and each
// fragment read is reused twice. Same transposed-staging/split-M/slab
// machinery as conv_wgrad_mfma_kernel.
// SCALED: min 3 waves/SIMD — the Sc8 registers pushed the allocation 4
// VGPRs over the 168 boundary (occ 3 -> 2, measured 1.77x slower)
template <typename T16, bool SCALED = false, bool KMIN = false>
__global__ __launch_bounds__(256, SCALED ? 3 : 2) void conv_wgrad_mfma_t128(
    const T16* __restrict__ x, const T16* __restrict__ dy,
    const float* __restrict__ asc,  // SCALED only
    const float* __restrict__ ash,
    float* __restrict__ dw,  // chunk slabs of [KO, R*S*CI]
    const int N, const int Hi, const int Wi, const int CI, const int KO,
    const int Ho, const int Wo, const int R, const int S, const int stride,
    const int pad, const long m_per_chunk, const int nchunks) {
  __shared__ T16 lds[(128 + 128) * LDM];

  const int tid = threadIdx.x;
  const long Mtot = (long)N * Ho * Wo;
  const int k0 = blockIdx.x * 128;
  const int cblocks = CI / 128;
  const int c0 = (blockIdx.y % cblocks) * 128;
  const int s_ = (blockIdx.y / cblocks) % S;
  const int r_ = blockIdx.y / (cblocks * S);
  const long m_begin = (long)blockIdx.z * m_per_chunk;
  const long m_end = min(Mtot, m_begin + m_per_chunk);

  // staging: all 256 threads stage dy (4m x 8k over 128 k-rows) and x
  // (4m x 8c over 128 c-rows) with the same (m-group, row-group) map.
  // KMIN: k-minor map + rotate-swizzled columns (see conv_wgrad_mfma_s3)
  const int sm = KMIN ? (tid >> 4) * 4 : (tid & 15) * 4;
  const int sk = KMIN ? (tid & 15) * 8 : (tid >> 4) * 8;

  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int li = lane & 31;
  const int kh = lane >> 5;
  const int i0 = (wave & 1) * 32;   // KO sub-offset
  const int j0 = (wave >> 1) * 32;  // CI sub-offset

  f32x16 acc[2][2] = {};
  Sc8 wsc{};
  if constexpr (SCALED) wsc = sc8_load(asc, ash, c0 + sk);

  int dn = 0, dp = 0, dq = 0;
  {
    const long m_first = m_begin + sm;
    dn = (int)(m_first / ((long)Ho * Wo));
    const int pq = (int)(m_first % ((long)Ho * Wo));
    dp = pq / Wo;
    dq = pq % Wo;
  }
  auto advance = [&](int by) {
    dq += by;
    while (dq >= Wo) {
      dq -= Wo;
      if (++dp == Ho) {
        dp = 0;
        ++dn;
      }
    }
  };

  short8 vdy[4], vx0[4];
  auto load_m = [&](long m0) {
    int n_ = dn, p_ = dp, q_ = dq;
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      const long m = m0 + sm + mi;
      vdy[mi] = m < m_end ? *reinterpret_cast<const short8*>(
                                dy + m * KO + k0 + sk)
                          : short8{};
      const int ih = p_ * stride - pad + r_;
      const int iw = q_ * stride - pad + s_;
      const bool ok = m < m_end && (unsigned)ih < (unsigned)Hi &&
                      (unsigned)iw < (unsigned)Wi;
      const T16* xp = x + (((long)n_ * Hi + ih) * Wi + iw) * CI + c0 + sk;
      vx0[mi] = ok ? *reinterpret_cast<const short8*>(xp) : short8{};
      if constexpr (SCALED) {
        if (ok) vx0[mi] = scale8<T16>(vx0[mi], wsc);
      }
      if (mi < 3 && ++q_ == Wo) {
        q_ = 0;
        if (++p_ == Ho) {
          p_ = 0;
          ++n_;
        }
      }
    }
    advance(WGM);
  };
  auto stage_m = [&]() {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int col = KMIN ? ((sm + ((sk + e) & 56)) & 63) : sm;
      short4v pk = {vdy[0][e], vdy[1][e], vdy[2][e], vdy[3][e]};
      *reinterpret_cast<short4v*>(
          reinterpret_cast<short*>(lds + (sk + e) * LDM + col)) = pk;
      short4v px0 = {vx0[0][e], vx0[1][e], vx0[2][e], vx0[3][e]};
      *reinterpret_cast<short4v*>(reinterpret_cast<short*>(
          lds + (128 + sk + e) * LDM + col)) = px0;
    }
  };

  load_m(m_begin);
  for (long m0 = m_begin; m0 < m_end; m0 += WGM) {
    __syncthreads();
    stage_m();
    __syncthreads();
    if (m0 + WGM < m_end) load_m(m0 + WGM);
    const T16* ldsDyT = lds;
    const T16* ldsXT = lds + 128 * LDM;
#pragma unroll
    for (int kk = 0; kk < WGM; kk += 16) {
      short8 af[2], bf[2];
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const int row = i0 + a * 64 + li;
        af[a] = *reinterpret_cast<const short8*>(
            ldsDyT + row * LDM +
            ((kk + kh * 8 + (KMIN ? (row & 56) : 0)) & 63));
      }
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int row = j0 + b * 64 + li;
        bf[b] = *reinterpret_cast<const short8*>(
            ldsXT + row * LDM +
            ((kk + kh * 8 + (KMIN ? (row & 56) : 0)) & 63));
      }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
          acc[a][b] = Mfma32<T16>::run(af[a], bf[b], acc[a][b]);
    }
  }

  const int rs = r_ * S + s_;
  const long RS = (long)R * S;
  float* slab = dw + (long)blockIdx.z * ((long)KO * CI * RS);
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int i = (reg & 3) + 8 * (reg >> 2) + 4 * kh;
        const int c_abs = c0 + j0 + b * 64 + li;
        slab[((long)(k0 + i0 + a * 64 + i) * CI + c_abs) * RS + rs] =
            acc[a][b][reg];
      }
}

// s-grouped wgrad for the dominant 3x3/stride-1/pad-1 convs: ONE block
// computes all 3 s-taps of one filter row r from ONE dy+x stage. The
// three x operand images are m-SHIFTED copies of the same center gather
// (x_im2col[m, s] = x_center[m + s - 1] within a q-row): each staging
// thread gathers 6 m-positions (4 + one halo on each side) and packs the
// three aligned 4-m transposed writes from its own registers, zeroing
// slots that cross a q-row boundary (q==0 for s=0, q==Wo-1 for s=2).
// Triples the MFMA work per staged dy/x byte — the plain kernel was
// staging-bound at ~190 TF while the fwd gather-GEMM reaches 470-670.
// KMIN (KT=64 only): k-minor staging-thread map + rotate-swizzled LDS
// columns — one wave's gather covers 8 full m-lines instead of 16
// quarter-lines (PMC: 53% parked on the gather latency), and the rotation
// keeps the transposed b64 writes bank-conflict-free where a plain
// k-minor map would collide 8-way (8*LDM elements = 0 mod 32 banks).
template <typename T16, int KT, bool SCALED = false, bool KMIN = false>
__global__ __launch_bounds__(256, SCALED ? 3 : 2) void conv_wgrad_mfma_s3(
    const T16* __restrict__ x,    // [N, Hi, Wi, CI]
    const T16* __restrict__ dy,   // [M, KO]
    const float* __restrict__ asc,  // SCALED only: [CI] lazy-BN scale
    const float* __restrict__ ash,
    float* __restrict__ dw,       // chunk slabs of [KO, 3*3*CI]
    const int N, const int Hi, const int Wi, const int CI, const int KO,
    const int Ho, const int Wo, const long m_per_chunk, const int nchunks) {
  __shared__ T16 lds[(KT + 3 * 64) * LDM];

  const int tid = threadIdx.x;
  const long Mtot = (long)N * Ho * Wo;
  const int k0 = blockIdx.x * KT;
  const int cchunks = CI / BK;
  const int c0 = (blockIdx.y % cchunks) * BK;
  const int r_ = blockIdx.y / cchunks;
  const long m_begin = (long)blockIdx.z * m_per_chunk;
  const long m_end = min(Mtot, m_begin + m_per_chunk);

  const bool do_dy = tid < 2 * KT;
  const bool do_x = KT == 64 ? tid >= 128 : tid < 128;
  const int t = do_dy ? tid : 0;
  const int sm = KMIN ? ((t >> 3) & 15) * 4 : (t & 15) * 4;
  const int sk = KMIN ? (t & 7) * 8 : (t >> 4) * 8;
  const int tx = tid & 127;
  const int smx = KMIN ? (tx >> 3) * 4 : (tx & 15) * 4;
  const int skx = KMIN ? (tx & 7) * 8 : (tx >> 4) * 8;

  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int li = lane & 31;
  const int kh = lane >> 5;
  constexpr int NJ = KT / 64;
  const int i0 = KT == 64 ? (wave & 1) * 32 : wave * 32;
  const int j0base = KT == 64 ? (wave >> 1) * 32 : 0;

  f32x16 acc[3][NJ] = {};
  Sc8 wsc{};
  if constexpr (SCALED) {
    if (do_x) wsc = sc8_load(asc, ash, c0 + skx);
  }

  // incremental decode for the CENTER gather position m = m0 + smx (the
  // i=0 halo position is derived from it: clamping a -1 start desyncs the
  // per-step advance for the smx==0 thread — measured as a wrong dw tile)
  int dn = 0, dp = 0, dq = 0;
  {
    const long m_first = m_begin + smx;
    dn = (int)(m_first / ((long)Ho * Wo));
    const int pq = (int)(m_first % ((long)Ho * Wo));
    dp = pq / Wo;
    dq = pq % Wo;
  }
  auto advance = [&](int by) {
    dq += by;
    while (dq >= Wo) {
      dq -= Wo;
      if (++dp == Ho) {
        dp = 0;
        ++dn;
      }
    }
  };

  short8 vdy[4], vx[6];
  int qg[6];  // q of each gathered position (for the row-boundary masks)
  auto load_m = [&](long m0) {
    if (do_dy) {
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
        const long m = m0 + sm + mi;
        vdy[mi] = (m < m_end) ? *reinterpret_cast<const short8*>(
                                    dy + m * KO + k0 + sk)
                              : short8{};
      }
    }
    if (do_x) {
      int n_ = dn, p_ = dp, q_ = dq;  // position m0 + smx (center start)
      {
        // i = 0 halo: column q-1 of the SAME row; when q == 0 the only
        // consumer slot (copy_0 at a q==0 target) is dead-masked, so a
        // zero stands in
        const int ih = p_ + r_ - 1;  // stride 1, pad 1
        qg[0] = q_ - 1;
        const bool ok = m0 + smx - 1 >= 0 && q_ > 0 &&
                        (unsigned)ih < (unsigned)Hi;
        vx[0] = ok ? *reinterpret_cast<const short8*>(
                         x + (((long)n_ * Hi + ih) * Wi + (q_ - 1)) * CI +
                         c0 + skx)
                   : short8{};
        if constexpr (SCALED) {
          if (ok) vx[0] = scale8<T16>(vx[0], wsc);
        }
      }
#pragma unroll
      for (int i = 1; i < 6; ++i) {
        const long m = m0 + smx - 1 + i;
        const int ih = p_ + r_ - 1;
        qg[i] = q_;
        const bool ok = m < Mtot && (unsigned)ih < (unsigned)Hi;
        vx[i] = ok ? *reinterpret_cast<const short8*>(
                         x + (((long)n_ * Hi + ih) * Wi + q_) * CI + c0 +
                         skx)
                   : short8{};
        if constexpr (SCALED) {
          if (ok) vx[i] = scale8<T16>(vx[i], wsc);
        }
        if (i < 5 && ++q_ == Wo) {
          q_ = 0;
          if (++p_ == Ho) {
            p_ = 0;
            ++n_;
          }
        }
      }
      advance(WGM);
    }
  };
  auto stage_m = [&]() {
    if (do_dy) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        short4v pk = {vdy[0][e], vdy[1][e], vdy[2][e], vdy[3][e]};
        const int col = KMIN ? ((sm + ((sk + e) & 56)) & 63) : sm;
        *reinterpret_cast<short4v*>(
            reinterpret_cast<short*>(lds + (sk + e) * LDM + col)) = pk;
      }
    }
    if (do_x) {
      // copy s slot j <- center gather index j + s; boundary slots zeroed
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        T16* ldsS = lds + (KT + s * 64) * LDM;
        short keep[4];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const int qt = qg[jj + 1];  // q of target output m
          const bool dead = (s == 0 && qt == 0) || (s == 2 && qt == Wo - 1);
          keep[jj] = dead ? (short)0 : (short)-1;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          short4v pk = {(short)(vx[s + 0][e] & keep[0]),
                        (short)(vx[s + 1][e] & keep[1]),
                        (short)(vx[s + 2][e] & keep[2]),
                        (short)(vx[s + 3][e] & keep[3])};
          const int col = KMIN ? ((smx + ((skx + e) & 56)) & 63) : smx;
          *reinterpret_cast<short4v*>(
              reinterpret_cast<short*>(ldsS + (skx + e) * LDM + col)) = pk;
        }
      }
    }
  };

  load_m(m_begin);
  for (long m0 = m_begin; m0 < m_end; m0 += WGM) {
    __syncthreads();
    stage_m();
    __syncthreads();
    if (m0 + WGM < m_end) load_m(m0 + WGM);
    const T16* ldsDyT = lds;
    const int arow = i0 + li;
    const int arot = KMIN ? (arow & 56) : 0;
#pragma unroll
    for (int kk = 0; kk < WGM; kk += 16) {
      const short8 af = *reinterpret_cast<const short8*>(
          ldsDyT + arow * LDM + ((kk + kh * 8 + arot) & 63));
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const T16* ldsXT = lds + (KT + s * 64) * LDM;
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
          const int brow = j0base + jj * 32 + li;
          const short8 bf = *reinterpret_cast<const short8*>(
              ldsXT + brow * LDM +
              ((kk + kh * 8 + (KMIN ? (brow & 56) : 0)) & 63));
          acc[s][jj] = Mfma32<T16>::run(af, bf, acc[s][jj]);
        }
      }
    }
  }

  float* slab = dw + (long)blockIdx.z * ((long)KO * CI * 9);
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const int rs = r_ * 3 + s;
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int i = (reg & 3) + 8 * (reg >> 2) + 4 * kh;
        const int c_abs = c0 + j0base + jj * 32 + li;
        slab[((long)(k0 + i0 + i) * CI + c_abs) * 9 + rs] = acc[s][jj][reg];
      }
    }
  }
}

// nine-tap wgrad for 3x3/stride-1/pad-1 convs whose 64-position m-step is
// a whole number of output rows inside one image (Wo in {8,16,32},
// Ho*Wo % 64 == 0), or four whole 4x4 images (below): ONE block computes
// all 9 taps of a 64(k) x 64(c) tile
// from ONE dy stage and ONE x stage per step, where the s3 kernel spends
// three blocks that each stage the same dy tile and a row-shifted copy of
// the same x rows. The x stage is the step's 64/Wo output rows plus one
// input row above and below, gathered once and written as three s-shifted
// transposed [c][position] images (position = input row * Wo + q, row 0 =
// the row above the step). A B fragment of tap (r, s) is image s read at
// position offset r*Wo: a whole-row offset, so every fragment read stays a
// 16-byte aligned ds_read_b128. Rows outside the image are staged as
// zeros; halo rows at a chunk boundary are ordinary rows of the same image
// and are loaded. The s shift comes from the neighbouring lane group (a
// wave stages 32 consecutive positions = whole rows), so each x element is
// requested from memory once per step.
// Both images use the k-minor staging map and rotate-swizzled columns of
// the s3 kernel; the x image is 128 columns wide so the rotation wraps
// with a mask.
// WO == 4 (Hi == 4 too, N % 4 == 0): a step is four whole images, still in
// natural position order. Input pixel (img, row, q) of the step sits at
// column img*24 + (row+1)*4 + q: every image has its own zero row above and
// below, zeroed once before the loop, so a step stages exactly its own 64
// positions and a thread's four positions are one whole image row (the
// q-1 / q+1 neighbours at its ends are the pad column: no lane exchange).
// The tap's row offset r*4 is 16-byte aligned for r = 0 and 2 only; the
// r = 1 fragment is put together from halves of those two.
constexpr int T9CL = 128;       // x image columns (>= 64 + 2*Wo, power of 2)
constexpr int T9LD = T9CL + 8;  // x image row length (+16B, as LDM)

template <typename T16, int WO>
__global__ __launch_bounds__(256, 2) void conv_wgrad_mfma_t9(
    const T16* __restrict__ x,   // [N, Hi, WO, CI]
    const T16* __restrict__ dy,  // [M, KO]
    float* __restrict__ dw,      // chunk slabs of [KO, 3*3*CI]
    const int Hi, const int CI, const int KO, const long Mtot,
    const long m_per_chunk) {
  constexpr bool IMG4 = WO == 4;
  static_assert(IMG4 || (WGM % WO == 0 && WO % 8 == 0 && 32 % WO == 0 &&
                         WGM + 2 * WO <= T9CL));
  // staged input positions per step
  constexpr int NPOS = IMG4 ? WGM : WGM + 2 * WO;
  __shared__ T16 lds[64 * LDM + 3 * 64 * T9LD];
  T16* const ldsX = lds + 64 * LDM;

  const int tid = threadIdx.x;
  const int k0 = blockIdx.x * 64;
  const int c0 = blockIdx.y * 64;
  const long m_begin = (long)blockIdx.z * m_per_chunk;
  const long m_end = min(Mtot, m_begin + m_per_chunk);

  // staging: the upper 128 threads stage dy (4 m x 8 k each); thread t
  // stages x positions 4*(t/8)..+3 x 8 channels while they are < NPOS
  const bool do_dy = tid >= 128;
  const int sm = ((tid & 127) >> 3) * 4;
  const int sk = (tid & 7) * 8;
  const int xpos = (tid >> 3) * 4;
  const bool do_x = xpos < NPOS;
  const int xi = xpos / WO;  // input row of the stage, 0 = row above
  const int xq = xpos % WO;

  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int li = lane & 31;
  const int kh = lane >> 5;
  const int i0 = (wave & 1) * 32;   // KO sub-tile
  const int j0 = (wave >> 1) * 32;  // CI sub-tile

  f32x16 acc[9] = {};

  // first output row of the step (steps never span images)
  int p0 = (int)((m_begin / WO) % Hi);

  short8 vdy[4], vx[4] = {};
  short xkeep = 0;  // 0 when this thread's input row lies outside the image
  auto load_m = [&](long m0) {
    if (do_dy) {
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
        vdy[mi] = *reinterpret_cast<const short8*>(
            dy + (m0 + sm + mi) * KO + k0 + sk);
    }
    if constexpr (IMG4) {
      if (do_x) {  // the step's own positions, nothing else
        const T16* xp = x + (m0 + xpos) * CI + c0 + sk;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          vx[j] = *reinterpret_cast<const short8*>(xp + (long)j * CI);
      }
      return;
    }
    if (do_x) {
      // Hi == Ho and Wi == Wo: pixel (n, p0, 0) has linear index m0, and
      // the stage's rows are contiguous from one row before it
      const bool ok = (unsigned)(p0 - 1 + xi) < (unsigned)Hi;
      xkeep = ok ? (short)-1 : (short)0;
      const T16* xp = x + (ok ? (m0 - WO + xpos) * CI : 0) + c0 + sk;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        vx[j] = *reinterpret_cast<const short8*>(xp + (long)j * CI);
    }
    p0 += WGM / WO;
    if (p0 >= Hi) p0 = 0;
  };
  auto stage_m = [&]() {
    if (do_dy) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        short4v pk = {vdy[0][e], vdy[1][e], vdy[2][e], vdy[3][e]};
        const int col = (sm + sk) & 63;  // (sk + e) & 56 == sk
        *reinterpret_cast<short4v*>(
            reinterpret_cast<short*>(lds + (sk + e) * LDM + col)) = pk;
      }
    }
    int4v hl{}, hr{};
    if constexpr (!IMG4) {
      // every lane runs the exchange (idle lanes carry unused values)
#pragma unroll
      for (int j = 0; j < 4; ++j) vx[j] &= xkeep;
      // q-1 of the first and q+1 of the last position: lane group -1 / +1
      // of the same wave; zero at the row ends (the pad column)
      hl = __builtin_bit_cast(int4v, vx[3]);
      hr = __builtin_bit_cast(int4v, vx[0]);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        hl[u] = __shfl_up(hl[u], 8, 64);
        hr[u] = __shfl_down(hr[u], 8, 64);
      }
    }
    if (do_x) {
      // WO == 4: the four positions are a whole row, both ends are pad
      const short8 zero{};
      const short8 vl =
          !IMG4 && xq > 0 ? __builtin_bit_cast(short8, hl) : zero;
      const short8 vr =
          !IMG4 && xq + 4 < WO ? __builtin_bit_cast(short8, hr) : zero;
      const int col =
          (IMG4 ? (xpos >> 4) * 24 + 4 + (xpos & 15) + sk : xpos + sk) &
          (T9CL - 1);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        short* row = reinterpret_cast<short*>(ldsX + (sk + e) * T9LD + col);
        short4v s0 = {vl[e], vx[0][e], vx[1][e], vx[2][e]};
        short4v s1 = {vx[0][e], vx[1][e], vx[2][e], vx[3][e]};
        short4v s2 = {vx[1][e], vx[2][e], vx[3][e], vr[e]};
        *reinterpret_cast<short4v*>(row) = s0;
        *reinterpret_cast<short4v*>(row + 64 * T9LD) = s1;
        *reinterpret_cast<short4v*>(row + 2 * 64 * T9LD) = s2;
      }
    }
  };

  if constexpr (IMG4) {
    // the zero rows of the four images: no stage writes them, so once
    const int c = tid & 63;
#pragma unroll
    for (int h = 0; h < 24; h += 20) {
      const int col = ((tid >> 6) * 24 + h + (c & 56)) & (T9CL - 1);
#pragma unroll
      for (int s = 0; s < 3; ++s)
        *reinterpret_cast<short4v*>(reinterpret_cast<short*>(
            ldsX + (s * 64 + c) * T9LD + col)) = short4v{};
    }
  }

  load_m(m_begin);
  for (long m0 = m_begin; m0 < m_end; m0 += WGM) {
    __syncthreads();
    stage_m();
    __syncthreads();
    if (m0 + WGM < m_end) load_m(m0 + WGM);
    const int arow = i0 + li;
    const int brow = j0 + li;
    const int acol = kh * 8 + (arow & 56);
    const int bcol = kh * 8 + (brow & 56);
    const T16* ap = lds + arow * LDM;
    const T16* bp = ldsX + brow * T9LD;
#pragma unroll
    for (int kk = 0; kk < WGM; kk += 16) {
      const short8 af =
          *reinterpret_cast<const short8*>(ap + ((kk + acol) & 63));
      if constexpr (IMG4) {
        // slice kk is image kk/16. The r = 1 fragment lies 8 bytes past the
        // r = 0 one and 8 bytes before the r = 2 one (no wrap can fall
        // inside it), so it is the upper half of one and the lower half of
        // the other: no read of its own, and none that is not 16-byte
        // aligned.
        const int col0 = ((kk / 16) * 24 + bcol) & (T9CL - 1);
        const int col2 = ((kk / 16) * 24 + 2 * WO + bcol) & (T9CL - 1);
#pragma unroll
        for (int s = 0; s < 3; ++s) {
          const T16* bs = bp + s * 64 * T9LD;
          const short8 b0 = *reinterpret_cast<const short8*>(bs + col0);
          const short8 b2 = *reinterpret_cast<const short8*>(bs + col2);
          const short8 b1 =
              __builtin_shufflevector(b0, b2, 4, 5, 6, 7, 8, 9, 10, 11);
          acc[s] = Mfma32<T16>::run(af, b0, acc[s]);
          acc[3 + s] = Mfma32<T16>::run(af, b1, acc[3 + s]);
          acc[6 + s] = Mfma32<T16>::run(af, b2, acc[6 + s]);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const int col = (kk + r * WO + bcol) & (T9CL - 1);
#pragma unroll
          for (int s = 0; s < 3; ++s) {
            const short8 bf = *reinterpret_cast<const short8*>(
                bp + s * 64 * T9LD + col);
            acc[r * 3 + s] = Mfma32<T16>::run(af, bf, acc[r * 3 + s]);
          }
        }
      }
    }
  }

  float* slab = dw + (long)blockIdx.z * ((long)KO * CI * 9);
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int i = (reg & 3) + 8 * (reg >> 2) + 4 * kh;
    float* o = slab + ((long)(k0 + i0 + i) * CI + c0 + j0 + li) * 9;
#pragma unroll
    for (int rs = 0; rs < 9; ++rs) o[rs] = acc[rs][reg];
  }
}

// out[zc][e] = sum over this block-row's z-range of part[z][e] — the
// z-parallel first level of the two-level reduce (small E can't fill the
// chip with element-parallelism alone)
__global__ void wgrad_reduce_zchunk(const float* __restrict__ part,
                                    float* __restrict__ out, long E, int nz,
                                    int z_per) {
  const int z0 = blockIdx.y * z_per;
  const int z1 = min(nz, z0 + z_per);
  long i0 = (long)(blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const long stride = (long)gridDim.x * blockDim.x * 4;
  for (long i = i0; i < E; i += stride) {
    if (i + 4 <= E) {
      float4v acc = *reinterpret_cast<const float4v*>(part + (long)z0 * E + i);
      for (int z = z0 + 1; z < z1; ++z) {
        float4v v = *reinterpret_cast<const float4v*>(part + (long)z * E + i);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] += v[u];
      }
      *reinterpret_cast<float4v*>(out + (long)blockIdx.y * E + i) = acc;
    } else {
      for (long e = i; e < E; ++e) {
        float a = part[(long)z0 * E + e];
        for (int z = z0 + 1; z < z1; ++z) a += part[(long)z * E + e];
        out[(long)blockIdx.y * E + e] = a;
      }
    }
  }
}

// dw[e] = sum_z part[z][e] (fp32, vectorized)
__global__ void wgrad_reduce_chunks(const float* __restrict__ part,
                                    float* __restrict__ dw, long E, int nz) {
  long i0 = (long)(blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const long stride = (long)gridDim.x * blockDim.x * 4;
  for (long i = i0; i < E; i += stride) {
    if (i + 4 <= E) {
      float4v acc = *reinterpret_cast<const float4v*>(part + i);
      for (int z = 1; z < nz; ++z) {
        float4v v = *reinterpret_cast<const float4v*>(part + (long)z * E + i);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] += v[u];
      }
      *reinterpret_cast<float4v*>(dw + i) = acc;
    } else {
      for (long e = i; e < E; ++e) {
        float a = part[e];
        for (int z = 1; z < nz; ++z) a += part[(long)z * E + e];
        dw[e] = a;
      }
    }
  }
}

}  // namespace

// host launchers --------------------------------------------------------
// One launch function per kernel family: it writes the argument list once
// and picks the compile-time variant. The variants are not full cross
// products; each pick<> lists exactly the ones that exist.

bool conv_mfma_supported(long CI, long KO) {
  return CI % 64 == 0 && KO % 64 == 0;
}

// 256-element zero page: out-of-bounds gathers SELECT this address instead
// of branching around the load — a per-element `ok ? load : 0` makes hipcc
// branch around each load and wait vmcnt(0) per element (guide §5 trap 4c:
// 32 dependent L2 round trips), which measured as ~1.5 us per OUTPUT in
// the stem kernels.
at::Tensor conv_zero_page(const at::Tensor& like) {
  static at::Tensor zp16, zph;
  at::Tensor& zp = like.scalar_type() == at::kBFloat16 ? zp16 : zph;
  if (!zp.defined() || zp.device() != like.device())
    zp = at::zeros({256}, like.options());
  return zp;
}

void wgrad_reduce_launch(at::Tensor part, at::Tensor dw, long E, long nz) {
  // Small E (stem filters: E ~ 9.4K) caps the element-parallel grid at a
  // handful of blocks — with thousands of slabs that left >95% of the chip
  // idle on a multi-hundred-MB reduction (measured: the stem wgrad was
  // ~5.6 ms END-TO-END of which the main kernel was a fraction — this
  // reduce was the rest). Two-level: z-chunked partial pass into [zc, E],
  // then the final single-pass sum.
  const int eblocks = (int)std::min<long>(cdiv_l(E, 256 * 4), 2048);
  long zc = std::min<long>(nz / 8, 2048 / std::max(eblocks, 1));
  if (zc > 1) {
    auto tmp = at::empty({zc, E}, part.options());
    const long per = cdiv_l(nz, zc);
    zc = cdiv_l(nz, per);
    launch256(wgrad_reduce_zchunk, dim3(eblocks, (unsigned)zc), 0,
              part.data_ptr<float>(), tmp.data_ptr<float>(), E, nz, per);
    launch256(wgrad_reduce_chunks, dim3(eblocks), 0, tmp.data_ptr<float>(),
              dw.data_ptr<float>(), E, zc);
    return;
  }
  launch256(wgrad_reduce_chunks, dim3(eblocks), 0, part.data_ptr<float>(),
            dw.data_ptr<float>(), E, nz);
}

namespace {

bool present(const at::Tensor& t) { return t.defined() && t.numel() > 0; }
float* f32_or_null(const at::Tensor& t) {
  return present(t) ? t.data_ptr<float>() : nullptr;
}

// knobs that more than one launcher reads
long wgrad_chunk_cap() {  // ablation knob: at most this many m-chunks
  static const long v = EnvKnob("MI355X_WGRAD_CHUNKS").num(0);
  return v;
}
bool conv_patch_on() {  // =0 falls back to the per-tap gather (fwd, dgrad)
  static const bool v = EnvKnob("MI355X_CONV_PATCH").on();
  return v;
}

// ---- wgrad ------------------------------------------------------------
// what the three wgrad kernel families share
struct WgradArgs {
  at::Tensor x, dy;
  const float *asc, *ash;  // lazy-BN transform of the x operand, or null
  int N, Hi, Wi, CI, KO, Ho, Wo, R, S, stride, pad;
};

// the staging variants that exist (there is no SCALED + KMIN kernel)
enum WgradMode { WG_PLAIN, WG_SCALED, WG_KMIN };
WgradMode wgrad_mode(const WgradArgs& a, bool kmin_knob) {
  return a.asc ? WG_SCALED : kmin_knob ? WG_KMIN : WG_PLAIN;
}

// Split-M plan of an MFMA wgrad: chunks of a multiple of WGM rows. One
// chunk stores straight into dw; several store one partial filter each,
// which wgrad_split_finish folds in order.
// A/B on layer1 b256 (partial slabs): m/chunk 1216 -> 189us, 4096 ->
// 137us, 16384 -> 327us: the lever is PER-CHUNK depth (~4096 m), which
// also holds as M grows with batch (576-total-blocks regressed b1024)
struct WgradSplit {
  long m_per_chunk;
  int nchunks;
  long E;
  at::Tensor part;
};
WgradSplit wgrad_split(long M, long E, const at::Tensor& dw, long cap,
                       long depth = 4096) {
  long want = std::min<long>(cdiv_l(M, depth), 4096);
  if (cap > 0) want = std::min(want, cap);
  const SplitPlan p = split_plan(M, want, WGM);
  return {p.per, (int)p.n, E,
          p.n > 1 ? at::empty({p.n, E}, dw.options()) : dw};
}
void wgrad_split_finish(const WgradSplit& sp, const at::Tensor& dw) {
  if (sp.nchunks > 1) wgrad_reduce_launch(sp.part, dw, sp.E, sp.nchunks);
}

// conv_wgrad_mfma_s3: KT=128 exists as the plain kernel only
void wgrad_s3_launch(const WgradArgs& a, int KT, WgradMode mode,
                     const WgradSplit& sp) {
  dim3 grid(a.KO / KT, 3 * (a.CI / 64), sp.nchunks);
  DISPATCH_16(a.x, T16, {
    auto go = [&](auto kern) {
      launch256(kern, grid, 0, (const T16*)a.x.data_ptr(),
                (const T16*)a.dy.data_ptr(), a.asc, a.ash,
                sp.part.data_ptr<float>(), a.N, a.Hi, a.Wi, a.CI, a.KO, a.Ho,
                a.Wo, sp.m_per_chunk, sp.nchunks);
    };
    if (KT == 128)
      go(conv_wgrad_mfma_s3<T16, 128>);
    else
      pick<WG_PLAIN, WG_SCALED, WG_KMIN>(mode, [&](auto m) {
        constexpr WgradMode M_ = decltype(m)::value;
        go(conv_wgrad_mfma_s3<T16, 64, M_ == WG_SCALED, M_ == WG_KMIN>);
      });
  });
}

// conv_wgrad_mfma_t9: one block per (k-tile, c-tile, chunk), all nine taps
bool wgrad_t9_eligible(const WgradArgs& a) {
  // a 64-position step is whole rows of one image, or four whole 4x4 images
  const bool rows = (a.Wo == 8 || a.Wo == 16 || a.Wo == 32) &&
                    (a.Ho * a.Wo) % WGM == 0;
  const bool img4 = a.Ho == 4 && a.Wo == 4 && ((long)a.N * 16) % WGM == 0;
  return a.R == 3 && a.S == 3 && a.stride == 1 && a.pad == 1 &&
         a.Hi == a.Ho && a.Wi == a.Wo && !a.asc && (rows || img4) &&
         a.KO % 64 == 0 && a.CI % 64 == 0;
}
void wgrad_t9_launch(const WgradArgs& a, const WgradSplit& sp) {
  dim3 grid(a.KO / 64, a.CI / 64, sp.nchunks);
  const long M = (long)a.N * a.Ho * a.Wo;
  DISPATCH_16(a.x, T16, {
    pick<4, 8, 16, 32>(a.Wo, [&](auto wo) {
      launch256(conv_wgrad_mfma_t9<T16, decltype(wo)::value>, grid, 0,
                (const T16*)a.x.data_ptr(), (const T16*)a.dy.data_ptr(),
                sp.part.data_ptr<float>(), a.Hi, a.CI, a.KO, M,
                sp.m_per_chunk);
    });
  });
}

void wgrad_t128_launch(const WgradArgs& a, WgradMode mode,
                       const WgradSplit& sp) {
  dim3 grid(a.KO / 128, (unsigned)(a.R * a.S * (a.CI / 128)), sp.nchunks);
  DISPATCH_16(a.x, T16, {
    pick<WG_PLAIN, WG_SCALED, WG_KMIN>(mode, [&](auto m) {
      constexpr WgradMode M_ = decltype(m)::value;
      launch256(conv_wgrad_mfma_t128<T16, M_ == WG_SCALED, M_ == WG_KMIN>,
                grid, 0, (const T16*)a.x.data_ptr(),
                (const T16*)a.dy.data_ptr(), a.asc, a.ash,
                sp.part.data_ptr<float>(), a.N, a.Hi, a.Wi, a.CI, a.KO, a.Ho,
                a.Wo, a.R, a.S, a.stride, a.pad, sp.m_per_chunk, sp.nchunks);
    });
  });
}

void wgrad_tap_launch(const WgradArgs& a, int KT, WgradMode mode,
                      const WgradSplit& sp) {
  dim3 grid(a.KO / KT, a.R * a.S * (a.CI / 64), sp.nchunks);
  DISPATCH_16(a.x, T16, {
    pick<128, 64>(KT, [&](auto kt) {
      pick<WG_PLAIN, WG_SCALED, WG_KMIN>(mode, [&](auto m) {
        constexpr WgradMode M_ = decltype(m)::value;
        launch256(conv_wgrad_mfma_kernel<T16, decltype(kt)::value,
                                         M_ == WG_SCALED, M_ == WG_KMIN>,
                  grid, 0, (const T16*)a.x.data_ptr(),
                  (const T16*)a.dy.data_ptr(), a.asc, a.ash,
                  sp.part.data_ptr<float>(), a.N, a.Hi, a.Wi, a.CI, a.KO,
                  a.Ho, a.Wo, a.R, a.S, a.stride, a.pad, sp.m_per_chunk,
                  sp.nchunks);
      });
    });
  });
}

}  // namespace

// asc/ash (optional): lazy-BN transform on the x operand (see fwd launcher)
void conv_wgrad_mfma_launch(at::Tensor x, at::Tensor dy, at::Tensor dw,
                            long R, long S, long stride, long pad,
                            at::Tensor asc, at::Tensor ash) {
  const float* asc_p = f32_or_null(asc);
  const WgradArgs a{x, dy, asc_p, asc_p ? f32_or_null(ash) : nullptr,
                    (int)x.size(0), (int)x.size(1), (int)x.size(2),
                    (int)x.size(3), (int)dy.size(3), (int)dy.size(1),
                    (int)dy.size(2), (int)R, (int)S, (int)stride, (int)pad};
  const long M = (long)a.N * a.Ho * a.Wo;
  const long E = (long)a.KO * R * S * a.CI;
  // nine taps per block where an m-step is whole output rows of one image
  // or four whole 4x4 images (MI355X_WGRAD_T9=0 restores the s3 path)
  static const bool t9_on = EnvKnob("MI355X_WGRAD_T9").on();
  if (t9_on && wgrad_t9_eligible(a)) {
    // Chunk depth stays at the s3 kernel's 4096 m: with the same chunks
    // every dw element is summed in the same order, so the result is bit
    // for bit the s3 kernel's. Deeper chunks are faster at large M (fewer
    // 147 KB partial slabs: b8192 layers 1/2/3 at 4096 / 8192 / 16384 m:
    // 928/906/882, 760/707/688, 751/694/669 us) but starve the chip at
    // small M (layer 1 at b256: 117 / 213 / 410 us) and change the order.
    static const long depth = EnvKnob("MI355X_T9_DEPTH").num(4096);
    const WgradSplit sp = wgrad_split(M, E, dw, wgrad_chunk_cap(),
                                      std::max<long>(depth, WGM));
    wgrad_t9_launch(a, sp);
    wgrad_split_finish(sp, dw);
    return;
  }
  // 3x3/s1/p1: s-grouped kernel (3 taps per stage) — MI355X_WGRAD_S3=0
  // falls back to the tap-per-block kernel
  static const bool s3_on = EnvKnob("MI355X_WGRAD_S3").on();
  if (s3_on && R == 3 && S == 3 && stride == 1 && pad == 1 && a.Hi == a.Ho &&
      a.Wi == a.Wo) {
    // A/B knob (r18: KT=64 90.98k vs KT=128 87.9k img/s). KT=64 default
    // even when KO%128==0: occupancy 3 vs 2 outweighs the wider tile's
    // staging amortization (measured +3.4% whole-bench)
    static const long ktf = EnvKnob("MI355X_WGRAD_S3_KT").num(0);
    // default ON (+0.5% r18, interleaved A/B x2); =0 disables
    static const bool kminor = EnvKnob("MI355X_S3_KMINOR").on();
    const int KT = (ktf == 128 && !asc_p) ? 128 : 64;  // scaled: KT=64 only
    const WgradSplit sp = wgrad_split(M, E, dw, wgrad_chunk_cap());
    wgrad_s3_launch(a, KT, wgrad_mode(a, kminor), sp);
    wgrad_split_finish(sp, dw);
    return;
  }
  // KO%128 && CI%128 (notably every r50 1x1 bottleneck conv): 128x128
  // output tile, 4 acc tiles per wave — 2x the MFMA per staged byte of
  // the 64-wide-CI kernel (which measured ~283 TF on these shapes)
  static const bool t128_on = EnvKnob("MI355X_WGRAD_T128").on();
  if (t128_on && a.KO % 128 == 0 && a.CI % 128 == 0) {
    // default ON (+0.8% r50, interleaved A/B x2)
    static const bool kmin128 = EnvKnob("MI355X_T128_KMINOR").on();
    const WgradSplit sp = wgrad_split(M, E, dw, 0);
    wgrad_t128_launch(a, wgrad_mode(a, kmin128), sp);
    wgrad_split_finish(sp, dw);
    return;
  }
  static const bool kming = EnvKnob("MI355X_WGRAD_KMINOR").on();
  const WgradSplit sp = wgrad_split(M, E, dw, wgrad_chunk_cap());
  wgrad_tap_launch(a, a.KO % 128 == 0 ? 128 : 64, wgrad_mode(a, kming), sp);
  wgrad_split_finish(sp, dw);
}

namespace {

// ---- fwd / dgrad ------------------------------------------------------
// conv_gather_gemm, all three uses: fwd (plain or SCALED), GENC fwd
// (NT=2 only) and dgrad (TRANS, plain or ADDIN). in/out are the GEMM's
// A-side and result tensors: (x, y) for fwd, (dy, dx) for dgrad.
// stats (optional, [2,KO], fully overwritten): the epilogue emits per-block
// (sum,sumsq) partials to a slab and stats_slab_reduce folds them.
void gather_gemm_launch(bool trans, bool genc, const at::Tensor& in,
                        const at::Tensor& wgt, const at::Tensor& bias,
                        const at::Tensor& addin, const float* asc,
                        const float* ash, at::Tensor& out,
                        const at::Tensor& stats, long R, long S, long stride,
                        long pad, long b_row_stride, long b_rs_stride,
                        long act) {
  const int N = in.size(0), Hi = in.size(1), Wi = in.size(2), CI = in.size(3);
  const int Ho = out.size(1), Wo = out.size(2), KO = out.size(3);
  const long M = (long)N * Ho * Wo;
  // BN=128 halves barriers per MFMA but also halves the grid — only use
  // it when M is large enough to keep the chip full at BM=128 tiles
  const bool wide =
      !genc && KO % 128 == 0 && cdiv_l(M, BM) * (KO / 128) >= 1024;
  const int nt = wide ? 4 : 2;
  dim3 grid((unsigned)cdiv_l(M, BM), KO / (nt * 32));
  at::Tensor zp = conv_zero_page(in);
  at::Tensor slab;
  if (present(stats))
    slab = at::empty({(long)grid.y * grid.x * 2 * nt * 32},
                     in.options().dtype(at::kFloat));
  DISPATCH_16(in, T16, {
    auto go = [&](auto kern) {
      launch256(kern, grid, 0, (const T16*)in.data_ptr(),
                (const T16*)wgt.data_ptr(), f32_or_null(bias),
                (const T16*)zp.data_ptr(),
                present(addin) ? (const T16*)addin.data_ptr() : nullptr, asc,
                ash, (T16*)out.data_ptr(), f32_or_null(slab), N, Hi, Wi, CI,
                KO, Ho, Wo, R, S, stride, pad, b_row_stride, b_rs_stride, act,
                present(bias));
    };
    if (genc)
      go(conv_gather_gemm<T16, false, true, 2>);
    else
      pick<4, 2>(nt, [&](auto NT) {
        if (trans)
          pick<true, false>(present(addin), [&](auto ADDIN) {
            go(conv_gather_gemm<T16, true, false, decltype(NT)::value,
                                decltype(ADDIN)::value>);
          });
        else
          pick<true, false>(asc != nullptr, [&](auto SCALED) {
            go(conv_gather_gemm<T16, false, false, decltype(NT)::value, false,
                                decltype(SCALED)::value>);
          });
      });
  });
  if (slab.defined()) stats_slab_reduce(slab, stats, grid.x, 2 * nt * 32, KO);
}

// LDS geometry of conv_patch_gemm for image width W: NR patch rows and the
// dynamic LDS bytes. NR = rows spanned by a 128-output tile starting
// mid-row, +2 halo rows: 128/W+3 was ONE short for W in {56,28,14,7} (tap
// r=2 then read past the patch -> diverging ResNet-50 training)
struct PatchGeom {
  int NR;
  size_t smem;
};
PatchGeom patch_geom(int W) {
  const int NR = (W + 126) / W + 3;
  return {NR, ((size_t)NR * (W + 2) * PCS + PCS + 64 * LDK) * 2};
}

// conv_patch_ring: one block per CU (MI355X_PATCH_RING_BLOCKS overrides the
// count), each walking images blockIdx.x, + gridDim.x, ...; the stats slab
// has one row per 128-output tile, as conv_patch_gemm's
void patch_ring_launch(bool trans, const at::Tensor& in,
                       const at::Tensor& wgt, const at::Tensor& bias,
                       const at::Tensor& addin, at::Tensor& out,
                       const at::Tensor& stats, long b_row_stride,
                       long b_rs_stride, long act) {
  const int N = in.size(0), Hi = in.size(1);
  const int KO = out.size(3);
  static const long blocks_knob = EnvKnob("MI355X_PATCH_RING_BLOCKS").num(0);
  const long blocks =
      blocks_knob > 0
          ? blocks_knob
          : at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  const long tiles = (long)N * Hi / 4;
  dim3 grid((unsigned)std::min<long>(N, blocks), KO / 64);
  at::Tensor slab;
  if (present(stats))
    slab = at::empty({(long)grid.y * tiles * 128},
                     in.options().dtype(at::kFloat));
  DISPATCH_16(in, T16, {
    auto go = [&](auto kern) {
      hipLaunchKernelGGL(
          kern, grid, dim3(512), 0, cur_stream(), (const T16*)in.data_ptr(),
          (const T16*)wgt.data_ptr(), f32_or_null(bias),
          present(addin) ? (const T16*)addin.data_ptr() : nullptr,
          (T16*)out.data_ptr(), f32_or_null(slab), N, Hi, KO, b_row_stride,
          b_rs_stride, (int)act, (int)present(bias));
    };
    if (trans)
      pick<true, false>(present(addin), [&](auto ADDIN) {
        go(conv_patch_ring<T16, true, decltype(ADDIN)::value>);
      });
    else
      go(conv_patch_ring<T16, false, false>);
  });
  if (slab.defined()) stats_slab_reduce(slab, stats, (int)tiles, 128, KO);
}

bool patch_ring_on() {
  static const bool v = EnvKnob("MI355X_PATCH_RING").on();
  return v;
}

// conv_patch_stream: one block per CU (MI355X_PATCH_STREAM_BLOCKS overrides
// the count; it is rounded down to a multiple of the KO/64 k-tiles, at
// least one block each). The blocks of a k-tile share its m-tiles of 256
// outputs; the stats slab has one row per 128-output tile, as
// conv_patch_gemm's.
void patch_stream_launch(bool trans, const at::Tensor& in,
                         const at::Tensor& wgt, const at::Tensor& bias,
                         const at::Tensor& addin, at::Tensor& out,
                         const at::Tensor& stats, long b_row_stride,
                         long b_rs_stride, long act) {
  const int N = in.size(0), Hi = in.size(1), Wi = in.size(2), CI = in.size(3);
  const int KO = out.size(3);
  static const long blocks_knob =
      EnvKnob("MI355X_PATCH_STREAM_BLOCKS").num(0);
  const long blocks =
      blocks_knob > 0
          ? blocks_knob
          : at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  const long M = (long)N * Hi * Wi;
  const long KT = KO / 64;
  const long MT = cdiv_l(M, ST_M);
  const long G = std::max(KT, std::min(MT * KT, blocks) / KT * KT);
  // blocks b and b + 8 share an XCD: where the counts allow it, a k-tile's
  // blocks are kept on as few XCDs as possible (the kernel's rank mapping)
  const bool xcd_local = G % 8 == 0 && 8 % KT == 0;
  int lw = 0;
  while ((1 << lw) < Wi) ++lw;
  const long nt128 = cdiv_l(M, 128);
  at::Tensor slab;
  if (present(stats))
    slab = at::empty({KT * nt128 * 128}, in.options().dtype(at::kFloat));
  DISPATCH_16(in, T16, {
    auto go = [&](auto kern) {
      hipLaunchKernelGGL(
          kern, dim3((unsigned)G), dim3(512), 0, cur_stream(),
          (const T16*)in.data_ptr(), (const T16*)wgt.data_ptr(),
          f32_or_null(bias),
          present(addin) ? (const T16*)addin.data_ptr() : nullptr,
          (T16*)out.data_ptr(), f32_or_null(slab), N, Hi, lw, CI, KO,
          b_row_stride, b_rs_stride, (int)act, (int)present(bias),
          (int)xcd_local);
    };
    if (trans)
      pick<true, false>(present(addin), [&](auto ADDIN) {
        go(conv_patch_stream<T16, true, decltype(ADDIN)::value>);
      });
    else
      go(conv_patch_stream<T16, false, false>);
  });
  if (slab.defined()) stats_slab_reduce(slab, stats, (int)nt128, 128, KO);
}

bool patch_stream_on() {
  static const bool v = EnvKnob("MI355X_PATCH_STREAM").on();
  return v;
}

// conv_patch_gemm (3x3/s1/p1, W <= 64): fwd (plain or SCALED, optional
// stats) and dgrad (TRANS, plain or ADDIN); in/out as in gather_gemm_launch.
// The 64-channel 32-wide layer goes to conv_patch_ring instead, and the
// layers of 128 channels and more at W = 4, 8 or 16 (whose 256-output tiles
// start at the beginning of an image row) to conv_patch_stream; every other
// width, ResNet-50's 56/28/14/7 among them, stays here.
void patch_gemm_launch(bool trans, const at::Tensor& in,
                       const at::Tensor& wgt, const at::Tensor& bias,
                       const at::Tensor& addin, const float* asc,
                       const float* ash, at::Tensor& out,
                       const at::Tensor& stats, long b_row_stride,
                       long b_rs_stride, long act) {
  const int N = in.size(0), Hi = in.size(1), Wi = in.size(2), CI = in.size(3);
  const int KO = out.size(3);
  if (patch_ring_on() && CI == 64 && KO % 64 == 0 && Wi == RG_W &&
      Hi % 4 == 0 && !asc) {
    patch_ring_launch(trans, in, wgt, bias, addin, out, stats, b_row_stride,
                      b_rs_stride, act);
    return;
  }
  if (patch_stream_on() && CI % 64 == 0 && CI >= 128 && KO % 64 == 0 &&
      (Wi == 4 || Wi == 8 || Wi == 16) && !asc) {
    patch_stream_launch(trans, in, wgt, bias, addin, out, stats, b_row_stride,
                        b_rs_stride, act);
    return;
  }
  const long M = (long)N * Hi * Wi;
  const PatchGeom pg = patch_geom(Wi);
  TORCH_CHECK(pg.smem >= (size_t)EpiTile<2>::BYTES,
              "patch LDS smaller than the epilogue's staged tile");
  dim3 grid((unsigned)cdiv_l(M, 128), KO / 64);
  at::Tensor slab;
  if (present(stats))
    slab = at::empty({(long)grid.y * grid.x * 128},
                     in.options().dtype(at::kFloat));
  DISPATCH_16(in, T16, {
    auto go = [&](auto kern) {
      launch256(kern, grid, pg.smem, (const T16*)in.data_ptr(),
                (const T16*)wgt.data_ptr(), f32_or_null(bias),
                present(addin) ? (const T16*)addin.data_ptr() : nullptr, asc,
                ash, (T16*)out.data_ptr(), f32_or_null(slab), N, Hi, Wi, CI,
                KO, b_row_stride, b_rs_stride, act, present(bias), pg.NR);
    };
    if (trans)
      pick<true, false>(present(addin), [&](auto ADDIN) {
        go(conv_patch_gemm<T16, true, decltype(ADDIN)::value>);
      });
    else
      pick<true, false>(asc != nullptr, [&](auto SCALED) {
        go(conv_patch_gemm<T16, false, false, decltype(SCALED)::value>);
      });
  });
  if (slab.defined()) stats_slab_reduce(slab, stats, grid.x, 128, KO);
}

// conv_dgrad_s2_gemm: the 4 parity classes ride in blockIdx.z
void dgrad_s2_launch(const at::Tensor& dy, const at::Tensor& wflip,
                     at::Tensor& dx, const at::Tensor& addin, long R, long S,
                     long pad) {
  const int N = dy.size(0), P = dy.size(1), Q = dy.size(2), KO = dy.size(3);
  const int H = dx.size(1), W = dx.size(2), CI = dx.size(3);
  const long Mmax = (long)N * ((H + 1) / 2) * ((W + 1) / 2);
  const bool wide = CI % 128 == 0 && cdiv_l(Mmax, BM) * (CI / 128) * 4 >= 1024;
  const int nt = wide ? 4 : 2;
  dim3 grid((unsigned)cdiv_l(Mmax, BM), CI / (nt * 32), 4);
  at::Tensor zp = conv_zero_page(dy);
  DISPATCH_16(dy, T16, {
    pick<4, 2>(nt, [&](auto NT) {
      pick<true, false>(present(addin), [&](auto ADDIN) {
        launch256(conv_dgrad_s2_gemm<T16, decltype(NT)::value,
                                     decltype(ADDIN)::value>,
                  grid, 0, (const T16*)dy.data_ptr(),
                  (const T16*)wflip.data_ptr(), (const T16*)zp.data_ptr(),
                  present(addin) ? (const T16*)addin.data_ptr() : nullptr,
                  (T16*)dx.data_ptr(), N, P, Q, KO, CI, H, W, R, S, pad);
      });
    });
  });
}

}  // namespace

// GENC fwd: wpad = [KO, KGP] zero-padded (cast_permute_krsc_pad)
void conv_fwd_mfma_genc_launch(at::Tensor x, at::Tensor wpad, at::Tensor bias,
                               at::Tensor y, long R, long S, long stride,
                               long pad, long act) {
  gather_gemm_launch(false, true, x, wpad, bias, at::Tensor(), nullptr,
                     nullptr, y, at::Tensor(), R, S, stride, pad,
                     wpad.size(1), 0, act);
}

// fwd: in = x[N,Hi,Wi,CI], wgt = w16 [KO, R,S,CI] row-major.
// stats (optional, [2,C], fully overwritten): conv->BN fusion — replaces
// BN's separate full-tensor bn_stats pass.
// asc/ash (optional [CI] fp32): lazy-BN A-side transform — the x operand
// is normalized+ReLU'd on load (z = relu(x*asc+ash)); the BN apply pass
// and its output tensor disappear.
void conv_fwd_mfma_launch(at::Tensor x, at::Tensor w, at::Tensor bias,
                          at::Tensor y, long stride, long pad, long act,
                          at::Tensor stats, at::Tensor asc, at::Tensor ash) {
  const float* asc_p = f32_or_null(asc);
  const float* ash_p = asc_p ? f32_or_null(ash) : nullptr;
  const long Hi = x.size(1), Wi = x.size(2), CI = x.size(3);
  const long R = w.size(1), S = w.size(2);
  // 3x3/s1/p1 patch kernel: one geometric LDS patch per c-chunk serves
  // all 9 taps
  if (conv_patch_on() && R == 3 && S == 3 && stride == 1 && pad == 1 &&
      y.size(1) == Hi && y.size(2) == Wi && Wi <= 64) {
    patch_gemm_launch(false, x, w, bias, at::Tensor(), asc_p, ash_p, y, stats,
                      R * S * CI, CI, act);
    return;
  }
  gather_gemm_launch(false, false, x, w, bias, at::Tensor(), asc_p, ash_p, y,
                     stats, R, S, stride, pad, R * S * CI, CI, act);
}

// dgrad: in = dy[N,P,Q,KO], wflip = [R,S,CI,KO] (w[k,R-1-r,S-1-s,c]),
// out = dx[N,H,W,CI]. addin (optional): dx = dgrad(dy) + addin — the
// residual-junction gradient fused into the epilogue (compile-time
// instantiation; the no-addin kernels are untouched).
void conv_dgrad_mfma_launch(at::Tensor dy, at::Tensor wflip, at::Tensor dx,
                            long R, long S, long stride, long pad,
                            at::Tensor addin) {
  const long KO = dy.size(3), CI = dx.size(3);
  // stride-2: parity-specialized kernel (4 classes in blockIdx.z), ~2.6x
  // fewer k-steps for 3x3/s2 and 4x for the 1x1 downsamples
  static const bool s2_on = EnvKnob("MI355X_DGRAD_S2").on();
  if (s2_on && stride == 2 && pad <= 8) {
    dgrad_s2_launch(dy, wflip, dx, addin, R, S, pad);
    return;
  }
  if (conv_patch_on() && R == 3 && S == 3 && stride == 1 && pad == 1 &&
      dy.size(1) == dx.size(1) && dy.size(2) == dx.size(2) &&
      dx.size(2) <= 64) {
    patch_gemm_launch(true, dy, wflip, at::Tensor(), addin, nullptr, nullptr,
                      dx, at::Tensor(), KO, CI * KO, 0);
    return;
  }
  gather_gemm_launch(true, false, dy, wflip, at::Tensor(), addin, nullptr,
                     nullptr, dx, at::Tensor(), R, S, stride, pad, KO,
                     CI * KO, 0);
}

