// Fused multi-head self-attention for image-classifier sequence lengths
// (1 <= S <= 256, head width 32 or 64, no mask, no dropout) over the packed
// output of the qkv projection, qkv[B,S,3,H,dh] in bf16 or fp16:
//
//   s_ij = sum_d q_id k_jd        P = softmax_j(scale * s)       o = P v
//
// o is [B,S,H*dh]; lse[B,H,S] = log sum_j exp(scale * s_ij) in fp32 is all
// the backward keeps besides qkv and o. The backward writes dqkv in the
// packed layout, every element of it.
//
// One block of four waves owns one (batch, head); the whole head is resident
// in LDS and registers, so scores and probabilities never reach HBM.
//
// Every product is computed TRANSPOSED, with the query on the MFMA column
// (= lane) axis: S^T = K Q^T leaves a lane with one query and, in its
// accumulator registers, that query's keys. The row maximum and the row sum
// are then register loops plus one or two cross-lane steps in a fixed order,
// and the same registers, rounded once to 16 bits, are directly the B operand
// of the second product O^T = V^T P^T (an MFMA k-slot may hold any key as long
// as both operands agree: the A operand reads V^T from LDS at the keys the
// accumulator layout dictates, two 8-byte reads). V (forward) and K
// (backward) are therefore kept transposed in LDS; rows from S to the bucket
// edge are zero-filled and columns >= S are excluded by select, never by
// arithmetic.
//
// MFMA form per sequence bucket: 32x32x16 for the 128 and 256 buckets (one
// LDS operand read feeds twice the FLOPs of the 16x16 form), 16x16x32 for
// S <= 64, where 32-row tiles would leave two of the four waves without a
// query tile (forward) or key tile (backward).
//
// Forward: K [SB][dh+8] and V^T [dh][SB+4] in LDS (16-byte global loads); a
// wave walks query tiles w, w+4, ...: Q fragments straight from HBM, S^T in
// NT accumulators, fp32 softmax with a true maximum (exp2 of
// (scale * s - scale * m) * log2 e), P rounded once, O^T, one division by
// the fp32 row sum, 8-byte stores.
//
// Backward: a wave owns key tiles w, w+4, ...; their K and V fragments stay
// in registers, dK^T and dV^T accumulate in registers over the 32-row query
// steps, which the block walks together in order. Per step: Q, dO (row-major
// and transposed) are staged in LDS; every wave forms S^T and dP^T of its
// keys and P = exp(scale * s - lse); D_i = sum_j P_ij dP_ij / sum_j P_ij
// (equal to sum_d dO_id o_id, without the roundings of o and of lse) is
// added over the waves in wave order; then S^T and dP^T again (cheaper than
// keeping them: the 256 bucket has no registers to spare) and
// dS = P (dP - D) in fp32; the wave rounds P and dS once and writes them to
// its own LDS tiles [key][query] (the
// transpose the dK/dV products need); dQ^T of the wave's keys goes to the
// wave's fp32 slot and the four slots are added in wave order, scaled,
// rounded and stored with 16-byte stores. No float atomics, no partial slabs
// in HBM: two runs give the same bits.
//
// Indices are decomposed in 32 bits; only element offsets are 64-bit. Every
// pointer argument is a real tensor's.
#include "common.h"

// no packed-fp32 instructions in this file (see gn.hip)
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

// No fused multiply-add by contraction: scale * s is rounded the same way
// where the forward takes the maximum, where it writes lse and where the
// backward recomputes P, so a one-token softmax is exactly 1 in both.
#pragma clang fp contract(off)

// AMfma, acc_row, ld16, cat4, kLog2e: shared with attn_flash.hip. Included
// here so that the helpers carry the two pragmas above.
#include "attn_mfma.h"

namespace {

template <int SB>
struct ATile {
  static constexpr int R = SB == 64 ? 16 : 32;  // MFMA tile edge
  static constexpr int NR = R * R / 64;         // accumulator registers
  static constexpr int KS = 512 / R;            // k-slots of one MFMA
  static constexpr int NT = SB / R;             // key tiles of the bucket
};

// ---- forward ----------------------------------------------------------------

template <typename T16, int DH, int SB>
__global__ __launch_bounds__(256) void attn_fwd_kernel(
    const T16* __restrict__ qkv, T16* __restrict__ o, float* __restrict__ lse,
    int S, int H, float scale) {
  using TL = ATile<SB>;
  constexpr int R = TL::R, NR = TL::NR, KS = TL::KS, NT = TL::NT;
  constexpr int NKD = DH / KS, DT = DH / R, CV = DH / 8;
  constexpr int KP = DH + 8, VP = SB + 4;  // LDS row pitches (elements)
  using M = AMfma<T16, R>;
  using Acc = typename M::acc;
  __shared__ __attribute__((aligned(16))) short Kl[SB * KP];
  __shared__ __attribute__((aligned(16))) short Vt[DH * VP];

  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const int li = lane % R, kg = lane / R;
  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  const int HD = H * DH;
  const long rs = 3L * HD;  // elements of one token of qkv
  const short* g =
      reinterpret_cast<const short*>(qkv) + (long)b * S * rs + h * DH;

  for (int idx = t; idx < SB * CV; idx += 256) {
    const int s = idx / CV, c = idx - s * CV;
    short8 kv = {}, vv = {};
    if (s < S) {
      kv = ld16(g + s * rs + HD + c * 8);
      vv = ld16(g + s * rs + 2 * HD + c * 8);
    }
    *reinterpret_cast<short8*>(&Kl[s * KP + c * 8]) = kv;
#pragma unroll
    for (int e = 0; e < 8; ++e) Vt[(c * 8 + e) * VP + s] = vv[e];
  }
  __syncthreads();

  for (int q0 = w * R; q0 < S; q0 += 4 * R) {
    const int qrow = q0 + li;
    short8 qf[NKD];
#pragma unroll
    for (int ks = 0; ks < NKD; ++ks) {
      qf[ks] = short8{};
      if (qrow < S) qf[ks] = ld16(g + qrow * rs + ks * KS + kg * 8);
    }
    // S^T: lane = query li, registers = keys
    Acc sc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      sc[j] = Acc{};
      if (j * R < S) {
#pragma unroll
        for (int ks = 0; ks < NKD; ++ks)
          sc[j] = M::run(ld16(&Kl[(j * R + li) * KP + ks * KS + kg * 8]),
                         qf[ks], sc[j]);
      }
    }
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < NR; ++r)
        if (j * R + acc_row(r, kg) < S) m = fmaxf(m, sc[j][r]);
#pragma unroll
    for (int off = R; off < 64; off <<= 1)
      m = fmaxf(m, __shfl_xor(m, off, kWave));
    float l = 0.f;
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const float p =
            j * R + acc_row(r, kg) < S
                ? exp2f((sc[j][r] * scale - m * scale) * kLog2e)
                : 0.f;
        sc[j][r] = p;
        l += p;
      }
#pragma unroll
    for (int off = R; off < 64; off <<= 1) l += __shfl_xor(l, off, kWave);

    // O^T = V^T P^T: the accumulator registers, eight at a time, are the B
    // operand; the A operand reads V^T at the keys those registers hold
    Acc oa[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) oa[dt] = Acc{};
#pragma unroll
    for (int f = 0; f < NT * NR / 8; ++f) {
      const int j0 = (8 * f) / NR, j1 = (8 * f + 4) / NR;
      if (j0 * R < S) {
        short8 pb;
#pragma unroll
        for (int e = 0; e < 8; ++e)
          pb[e] = f32_to_s16<T16>(sc[(8 * f + e) / NR][(8 * f + e) % NR]);
        const int key0 = j0 * R + acc_row((8 * f) % NR, kg);
        const int key1 = j1 * R + acc_row((8 * f + 4) % NR, kg);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          const short* row = &Vt[(dt * R + li) * VP];
          oa[dt] = M::run(cat4(row + key0, row + key1), pb, oa[dt]);
        }
      }
    }
    if (qrow < S) {
      const float inv = 1.f / l;
      short* op = reinterpret_cast<short*>(o) + ((long)b * S + qrow) * HD +
                  h * DH;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int g4 = 0; g4 < NR / 4; ++g4) {
          short4v v;
#pragma unroll
          for (int u = 0; u < 4; ++u)
            v[u] = f32_to_s16<T16>(oa[dt][g4 * 4 + u] * inv);
          *reinterpret_cast<short4v*>(op + dt * R + 8 * g4 + 4 * kg) = v;
        }
      if (kg == 0)
        lse[((long)b * H + h) * S + qrow] = m * scale + logf(l);
    }
  }
}

// ---- backward ---------------------------------------------------------------

template <typename T16, int DH, int SB>
__global__ __launch_bounds__(256) void attn_bwd_kernel(
    const T16* __restrict__ qkv, const T16* __restrict__ o,
    const float* __restrict__ lse, const T16* __restrict__ dout,
    T16* __restrict__ dqkv, int S, int H, float scale) {
  using TL = ATile<SB>;
  constexpr int R = TL::R, NR = TL::NR, KS = TL::KS;
  constexpr int KPW = TL::NT / 4;  // key tiles of a wave
  constexpr int TQ = 32;           // query rows of a step
  constexpr int QS = TQ / R, NKD = DH / KS, NKQ = TQ / KS, DT = DH / R;
  constexpr int CV = DH / 8;
  constexpr int KTP = SB + 4, QP = DH + 8, TP = TQ + 8, DQP = DH + 4;
  constexpr int NF = (KPW * NR + 7) / 8;  // B fragments of a wave's dS
  using M = AMfma<T16, R>;
  using Acc = typename M::acc;
  __shared__ __attribute__((aligned(16))) short Kt[DH * KTP];
  __shared__ __attribute__((aligned(16))) short Ql[TQ * QP], dOl[TQ * QP];
  __shared__ __attribute__((aligned(16))) short Qt[DH * TP], dOt[DH * TP];
  __shared__ __attribute__((aligned(16))) short Pl[4 * KPW * R * TP];
  __shared__ __attribute__((aligned(16))) short dSl[4 * KPW * R * TP];
  __shared__ __attribute__((aligned(16))) float dQp[4 * TQ * DQP];
  __shared__ float Ll[TQ], Dp[4 * TQ], Zp[4 * TQ];

  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const int li = lane % R, kg = lane / R;
  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  const int HD = H * DH;
  const long rs = 3L * HD;
  const long tok0 = (long)b * S;
  const short* g = reinterpret_cast<const short*>(qkv) + tok0 * rs + h * DH;
  const short* dg = reinterpret_cast<const short*>(dout) + tok0 * HD + h * DH;
  short* dqg = reinterpret_cast<short*>(dqkv) + tok0 * rs + h * DH;
  const float* lg = lse + ((long)b * H + h) * S;

  for (int idx = t; idx < SB * CV; idx += 256) {
    const int s = idx / CV, c = idx - s * CV;
    short8 kv = {};
    if (s < S) kv = ld16(g + s * rs + HD + c * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) Kt[(c * 8 + e) * KTP + s] = kv[e];
  }
  // the wave's keys: K and V fragments in registers for the whole kernel
  short8 kf[KPW][NKD], vf[KPW][NKD];
  Acc dkt[KPW][DT], dvt[KPW][DT];
#pragma unroll
  for (int jj = 0; jj < KPW; ++jj) {
    const int key = (w + 4 * jj) * R + li;
#pragma unroll
    for (int ks = 0; ks < NKD; ++ks) {
      kf[jj][ks] = short8{};
      vf[jj][ks] = short8{};
      if (key < S) {
        kf[jj][ks] = ld16(g + key * rs + HD + ks * KS + kg * 8);
        vf[jj][ks] = ld16(g + key * rs + 2 * HD + ks * KS + kg * 8);
      }
    }
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      dkt[jj][dt] = Acc{};
      dvt[jj][dt] = Acc{};
    }
  }

  for (int q0 = 0; q0 < S; q0 += TQ) {
    // stage Q, dO (both ways round), D and lse of the step
    if (t < TQ * CV) {
      const int row = t / CV, c = t - row * CV;
      const int qrow = q0 + row;
      short8 qv = {}, dv = {};
      if (qrow < S) {
        qv = ld16(g + qrow * rs + c * 8);
        dv = ld16(dg + (long)qrow * HD + c * 8);
      }
      *reinterpret_cast<short8*>(&Ql[row * QP + c * 8]) = qv;
      *reinterpret_cast<short8*>(&dOl[row * QP + c * 8]) = dv;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        Qt[(c * 8 + e) * TP + row] = qv[e];
        dOt[(c * 8 + e) * TP + row] = dv[e];
      }
      if (c == 0) Ll[row] = qrow < S ? lg[qrow] : 0.f;
    }
    __syncthreads();

    // S^T and dP^T of one of the wave's key tiles against a query sub-tile
    auto products = [&](int jj, int qs, Acc& st, Acc& dpt) {
      const int ql = qs * R + li;
#pragma unroll
      for (int ks = 0; ks < NKD; ++ks) {
        st = M::run(kf[jj][ks], ld16(&Ql[ql * QP + ks * KS + kg * 8]), st);
        dpt = M::run(vf[jj][ks], ld16(&dOl[ql * QP + ks * KS + kg * 8]), dpt);
      }
    };
    // D_q = sum_j P_qj dP_qj / sum_j P_qj (= sum_d dO_qd o_qd, but from the
    // fp32 P: the rounding of o does not enter, and where P is a single 1
    // dP - D cancels exactly). The recomputed row sums to 1 + e, e from the
    // rounding of lse (3.8e-6 where |lse| is 80); dividing by it keeps
    // dS = P (dP - D) a multiple of the exact one, where P (dP - sum P dP)
    // would leave -e P D behind wherever dP - D cancels. The wave's keys in
    // registers, the lane groups by shuffle, the waves through LDS in wave
    // order.
    float Dq[QS], Zq[QS];
#pragma unroll
    for (int qs = 0; qs < QS; ++qs) Dq[qs] = Zq[qs] = 0.f;
#pragma unroll
    for (int jj = 0; jj < KPW; ++jj) {
      const int k0 = (w + 4 * jj) * R;
      if (k0 < S) {
#pragma unroll
        for (int qs = 0; qs < QS; ++qs) {
          const int ql = qs * R + li;
          Acc st = {}, dpt = {};
          products(jj, qs, st, dpt);
          const float L = Ll[ql];
#pragma unroll
          for (int r = 0; r < NR; ++r)
            if (q0 + ql < S && k0 + acc_row(r, kg) < S) {
              const float p = exp2f((st[r] * scale - L) * kLog2e);
              Zq[qs] += p;
              Dq[qs] += p * dpt[r];
            }
        }
      }
    }
#pragma unroll
    for (int qs = 0; qs < QS; ++qs) {
#pragma unroll
      for (int off = R; off < 64; off <<= 1) {
        Dq[qs] += __shfl_xor(Dq[qs], off, kWave);
        Zq[qs] += __shfl_xor(Zq[qs], off, kWave);
      }
      if (kg == 0) {
        Dp[w * TQ + qs * R + li] = Dq[qs];
        Zp[w * TQ + qs * R + li] = Zq[qs];
      }
    }
    __syncthreads();
#pragma unroll
    for (int qs = 0; qs < QS; ++qs) {
      const int ql = qs * R + li;
      const float z =
          ((Zp[ql] + Zp[TQ + ql]) + Zp[2 * TQ + ql]) + Zp[3 * TQ + ql];
      Dq[qs] = ((Dp[ql] + Dp[TQ + ql]) + Dp[2 * TQ + ql]) + Dp[3 * TQ + ql];
      Dq[qs] = q0 + ql < S ? Dq[qs] / z : 0.f;  // rows past S: z = 0
    }

    // S^T, dP^T, P and dS of the wave's keys against the step's queries
    short8 dsr[QS][NF];  // the rounded dS, packed as the dQ B fragments
#pragma unroll
    for (int qs = 0; qs < QS; ++qs)
#pragma unroll
      for (int f = 0; f < NF; ++f) dsr[qs][f] = short8{};
#pragma unroll
    for (int jj = 0; jj < KPW; ++jj) {
      const int k0 = (w + 4 * jj) * R;
      if (k0 < S) {
        short* pl = &Pl[(w * KPW + jj) * R * TP];
        short* dsl = &dSl[(w * KPW + jj) * R * TP];
#pragma unroll
        for (int qs = 0; qs < QS; ++qs) {
          const int ql = qs * R + li;
          Acc st = {}, dpt = {};
          products(jj, qs, st, dpt);
          const float L = Ll[ql];
          const bool qok = q0 + ql < S;
#pragma unroll
          for (int r = 0; r < NR; ++r) {
            const int kl = acc_row(r, kg);
            const bool ok = qok && k0 + kl < S;
            const float p = ok ? exp2f((st[r] * scale - L) * kLog2e) : 0.f;
            const float ds = ok ? p * (dpt[r] - Dq[qs]) : 0.f;
            const short ds16 = f32_to_s16<T16>(ds);
            pl[kl * TP + ql] = f32_to_s16<T16>(p);
            dsl[kl * TP + ql] = ds16;
            dsr[qs][(jj * NR + r) / 8][(jj * NR + r) % 8] = ds16;
          }
        }
      }
    }
    // dQ^T of the wave's keys: B = the rounded dS registers, A = K^T
    Acc dqt[DT][QS];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int qs = 0; qs < QS; ++qs) dqt[dt][qs] = Acc{};
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const int i0 = 8 * f, i1 = 8 * f + 4 < KPW * NR ? 8 * f + 4 : 8 * f;
      const int key0 = (w + 4 * (i0 / NR)) * R + acc_row(i0 % NR, kg);
      const int key1 = (w + 4 * (i1 / NR)) * R + acc_row(i1 % NR, kg);
      if ((w + 4 * (i0 / NR)) * R < S) {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          const short* row = &Kt[(dt * R + li) * KTP];
          const short8 a = cat4(row + key0, row + key1);
#pragma unroll
          for (int qs = 0; qs < QS; ++qs)
            dqt[dt][qs] = M::run(a, dsr[qs][f], dqt[dt][qs]);
        }
      }
    }
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int qs = 0; qs < QS; ++qs)
#pragma unroll
        for (int g4 = 0; g4 < NR / 4; ++g4) {
          float4v v;
#pragma unroll
          for (int u = 0; u < 4; ++u) v[u] = dqt[dt][qs][g4 * 4 + u];
          *reinterpret_cast<float4v*>(
              &dQp[(w * TQ + qs * R + li) * DQP + dt * R + 8 * g4 + 4 * kg]) =
              v;
        }
    __syncthreads();

    // dV^T += dO^T P, dK^T += Q^T dS over the step's queries
#pragma unroll
    for (int jj = 0; jj < KPW; ++jj) {
      if ((w + 4 * jj) * R < S) {
        const short* pl = &Pl[(w * KPW + jj) * R * TP + li * TP];
        const short* dsl = &dSl[(w * KPW + jj) * R * TP + li * TP];
#pragma unroll
        for (int ks = 0; ks < NKQ; ++ks) {
          const short8 bp = ld16(pl + ks * KS + kg * 8);
          const short8 bd = ld16(dsl + ks * KS + kg * 8);
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) {
            const int ao = (dt * R + li) * TP + ks * KS + kg * 8;
            dvt[jj][dt] = M::run(ld16(&dOt[ao]), bp, dvt[jj][dt]);
            dkt[jj][dt] = M::run(ld16(&Qt[ao]), bd, dkt[jj][dt]);
          }
        }
      }
    }
    // dQ: the four waves' slots in wave order
    if (t < TQ * CV) {
      const int row = t / CV, c = t - row * CV;
      if (q0 + row < S) {
        float a[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) a[u] = dQp[row * DQP + c * 8 + u];
#pragma unroll
        for (int ww = 1; ww < 4; ++ww)
#pragma unroll
          for (int u = 0; u < 8; ++u)
            a[u] += dQp[(ww * TQ + row) * DQP + c * 8 + u];
        short8 v;
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = f32_to_s16<T16>(a[u] * scale);
        *reinterpret_cast<short8*>(dqg + (q0 + row) * rs + c * 8) = v;
      }
    }
    __syncthreads();
  }

#pragma unroll
  for (int jj = 0; jj < KPW; ++jj) {
    const int key = (w + 4 * jj) * R + li;
    if (key < S) {
      short* kp = dqg + key * rs + HD;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int g4 = 0; g4 < NR / 4; ++g4) {
          short4v vk, vv;
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            vk[u] = f32_to_s16<T16>(dkt[jj][dt][g4 * 4 + u] * scale);
            vv[u] = f32_to_s16<T16>(dvt[jj][dt][g4 * 4 + u]);
          }
          const int d = dt * R + 8 * g4 + 4 * kg;
          *reinterpret_cast<short4v*>(kp + d) = vk;
          *reinterpret_cast<short4v*>(kp + HD + d) = vv;
        }
    }
  }
}

#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif

// ---- host -------------------------------------------------------------------

struct AttnDims {
  int B, S, H, dh;
  int cfg;  // dh * 1000 + sequence bucket
};

AttnDims attn_dims(const at::Tensor& qkv) {
  CHECK_GPU(qkv);
  CHECK_CONTIG(qkv);
  CHECK_16BIT(qkv);
  TORCH_CHECK(qkv.dim() == 5 && qkv.size(2) == 3,
              "attention: qkv must be [B,S,3,H,dh]");
  const long B = qkv.size(0), S = qkv.size(1), H = qkv.size(3),
             dh = qkv.size(4);
  TORCH_CHECK(dh == 32 || dh == 64, "attention: head width=", dh,
              " must be 32 or 64");
  TORCH_CHECK(S >= 1 && S <= 256, "attention: sequence length=", S,
              " must be in [1, 256]");
  TORCH_CHECK(B >= 1 && H >= 1 && B * H < (1L << 31) && H * dh < (1L << 20),
              "attention: batch or head count too large");
  const int bucket = S <= 64 ? 64 : S <= 128 ? 128 : 256;
  return AttnDims{(int)B, (int)S, (int)H, (int)dh, (int)dh * 1000 + bucket};
}

}  // namespace

// returns {o[B,S,H*dh], lse[B,H,S]}
std::vector<at::Tensor> attn_fwd(at::Tensor qkv, double scale) {
  const AttnDims d = attn_dims(qkv);
  auto o = at::empty({d.B, d.S, (long)d.H * d.dh}, qkv.options());
  auto lse = at::empty({d.B, d.H, d.S}, qkv.options().dtype(at::kFloat));
  DISPATCH_16(qkv, T16, {
    pick<32064, 32128, 32256, 64064, 64128, 64256>(d.cfg, [&](auto CFG) {
      launch256(
          (attn_fwd_kernel<T16, decltype(CFG)::value / 1000,
                           decltype(CFG)::value % 1000>),
          dim3((unsigned)(d.B * d.H)), 0, (const T16*)qkv.data_ptr(),
          (T16*)o.data_ptr(), lse.data_ptr<float>(), d.S, d.H, (float)scale);
    });
  });
  return {o, lse};
}

// returns dqkv[B,S,3,H,dh], every element written
at::Tensor attn_bwd(at::Tensor qkv, at::Tensor o, at::Tensor lse,
                    at::Tensor dout, double scale) {
  const AttnDims d = attn_dims(qkv);
  const long D = (long)d.H * d.dh;
  for (const at::Tensor* x : {&o, &dout})
    TORCH_CHECK(x->is_cuda() && x->is_contiguous() &&
                    x->scalar_type() == qkv.scalar_type() && x->dim() == 3 &&
                    x->size(0) == d.B && x->size(1) == d.S && x->size(2) == D,
                "attention: o and do must be contiguous [B,S,H*dh] of qkv's "
                "dtype");
  TORCH_CHECK(lse.is_cuda() && lse.is_contiguous() &&
                  lse.scalar_type() == at::kFloat &&
                  lse.numel() == (long)d.B * d.H * d.S,
              "attention: lse must be fp32 [B,H,S]");
  auto dqkv = at::empty_like(qkv);
  DISPATCH_16(qkv, T16, {
    pick<32064, 32128, 32256, 64064, 64128, 64256>(d.cfg, [&](auto CFG) {
      launch256(
          (attn_bwd_kernel<T16, decltype(CFG)::value / 1000,
                           decltype(CFG)::value % 1000>),
          dim3((unsigned)(d.B * d.H)), 0, (const T16*)qkv.data_ptr(),
          (const T16*)o.data_ptr(), lse.data_ptr<float>(),
          (const T16*)dout.data_ptr(), (T16*)dqkv.data_ptr(), d.S, d.H,
          (float)scale);
    });
  });
  return dqkv;
}
