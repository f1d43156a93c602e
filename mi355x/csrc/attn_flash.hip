// Streaming multi-head self-attention for sequence lengths past the resident
// kernels of attn.hip: 1 <= S <= 4096, head width 32 or 64, no mask, no
// dropout, over the packed qkv[B,S,3,H,dh] in bf16 or fp16:
//
//   s_ij = sum_d q_id k_jd        P = softmax_j(scale * s)       o = P v
//
// o is [B,S,H*dh]; lse[B,H,S] in fp32 is all the backward keeps besides qkv
// (not even o: see D below). The backward writes every element of dqkv.
//
// The products keep attn.hip's orientation: the query sits on the MFMA column
// (= lane) axis, S^T = K Q^T, so one lane owns one query and its accumulator
// registers hold that query's keys. The online-softmax state of a query (the
// running maximum m and the running sum l) is therefore two scalars of a lane
// pair, the rescaling of O^T by alpha is one multiply per accumulator register
// with no broadcast, and the probabilities, rounded once to 16 bits in the
// accumulator registers, are directly the B operand of O^T += V^T P^T (the A
// operand reads V^T from LDS at the keys the accumulator layout dictates).
//
// Forward, flash_fwd_kernel: a block of four waves owns 128 queries of one
// (batch, head), a wave 32 of them on 32x32x16 MFMA; the Q fragments stay in
// registers. The query tile is the fastest block index, so the blocks of a
// head run together and its K/V stay in L2. Keys stream in tiles of 64
// through double-buffered LDS, K [64][dh+8] and V^T [dh][64+4]: the next
// tile's 16-byte global loads are issued before the current tile's MFMAs and
// written to the other buffer after them, one barrier per tile. Per tile:
// m' = max(m, tile max), alpha = exp2((m scale - m' scale) log2 e),
// l = l alpha + sum p, O^T *= alpha, p = exp2((s scale - m' scale) log2 e)
// without FMA contraction (a one-token softmax is exactly 1 and
// lse = m scale + logf(l) rounds as the backward recomputes it). l is kept
// per lane and the two lanes of a query meet once, at the end. Keys >= S are
// excluded by select, never by arithmetic; rows past S are zero-filled.
//
// Backward, two kernels. D_i = sum_j P_ij dP_ij / sum_j P_ij comes from the
// recomputed fp32 P, never from the 16-bit o (profiles/r17_attention.md).
//
// flash_bwd_dq_kernel: grid and wave split of the forward; Q and dO fragments
// in registers; key tiles carry K, V (row-major) and K^T. Two sweeps over the
// keys in one launch and one pipeline: the first forms S^T, dP^T = V dO^T and
// P = exp(scale s - lse) and adds P dP and P per lane, which gives D (written
// as fp32 [B,H,S] for the second kernel); the second recomputes them, forms
// dS = P (dP - D) in fp32, rounds it once, and those registers are the B
// operand of dQ^T += K^T dS^T. dq = scale dQ is rounded once.
//
// flash_bwd_dkv_kernel: a block owns 128 keys, a wave 32; their K and V
// fragments and the dK^T, dV^T accumulators stay in registers. The block
// walks query steps of 32 in order through double-buffered LDS (Q and dO
// row-major and transposed, lse and D of the step). Here the products are
// formed UNtransposed, lane = key and registers = queries: S = Q K^T,
// dP = dO V^T, so that the rounded P and dS registers are directly the B
// operands of dV^T += dO^T P and dK^T += Q^T dS, with no LDS round trip.
//
// No float atomics, no scratch that grows with S^2 (D is [B,H,S]), a fixed
// order in every sum: two runs give the same bits. Indices are decomposed in
// 32 bits; only element offsets are 64-bit. Every pointer argument is a real
// tensor's.
#include "common.h"

// no packed-fp32 instructions in this file (see gn.hip)
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

// No fused multiply-add by contraction: scale * s is rounded the same way
// where the forward takes the maximum, where it writes lse and where the
// backward recomputes P.
#pragma clang fp contract(off)

#include "attn_mfma.h"

namespace {

constexpr int kTQ = 128;  // queries (forward, dq) or keys (dkv) of a block
constexpr int kTK = 64;   // keys of a streamed tile
constexpr int kQS = 32;   // queries of a dkv step
constexpr int kR = 32;    // MFMA tile edge
constexpr int kNR = 16;   // accumulator registers of a tile
constexpr int kKS = 16;   // k-slots of one MFMA

// ---- forward ----------------------------------------------------------------

template <typename T16, int DH>
__global__ __launch_bounds__(256) void flash_fwd_kernel(
    const T16* __restrict__ qkv, T16* __restrict__ o, float* __restrict__ lse,
    int S, int H, int nqt, float scale) {
  constexpr int NKD = DH / kKS, DT = DH / kR, CV = DH / 8;
  constexpr int KP = DH + 8, VP = kTK + 4;  // LDS row pitches (elements)
  constexpr int NLD = kTK * CV / 256;       // 16-byte chunks a thread stages
  constexpr int NJ = kTK / kR;              // 32-key sub-tiles of a tile
  using M = AMfma<T16, kR>;
  using Acc = typename M::acc;
  __shared__ __attribute__((aligned(16))) short Kl[2][kTK * KP];
  __shared__ __attribute__((aligned(16))) short Vt[2][DH * VP];

  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const int li = lane % kR, kg = lane / kR;
  const int bh = blockIdx.x / nqt, qt = blockIdx.x - bh * nqt;
  const int b = bh / H, h = bh - b * H;
  const int HD = H * DH;
  const long rs = 3L * HD;  // elements of one token of qkv
  const short* g =
      reinterpret_cast<const short*>(qkv) + (long)b * S * rs + h * DH;
  const int qrow = qt * kTQ + w * kR + li;
  const bool live = qt * kTQ + w * kR < S;  // the wave has a query

  short8 qf[NKD];
#pragma unroll
  for (int ks = 0; ks < NKD; ++ks) {
    qf[ks] = short8{};
    if (qrow < S) qf[ks] = ld16(g + qrow * rs + ks * kKS + kg * 8);
  }

  short8 kr[NLD], vr[NLD];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int idx = t + i * 256, s = idx / CV, c = idx - s * CV;
      kr[i] = short8{};
      vr[i] = short8{};
      if (k0 + s < S) {
        kr[i] = ld16(g + (k0 + s) * rs + HD + c * 8);
        vr[i] = ld16(g + (k0 + s) * rs + 2 * HD + c * 8);
      }
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int idx = t + i * 256, s = idx / CV, c = idx - s * CV;
      *reinterpret_cast<short8*>(&Kl[buf][s * KP + c * 8]) = kr[i];
#pragma unroll
      for (int e = 0; e < 8; ++e) Vt[buf][(c * 8 + e) * VP + s] = vr[i][e];
    }
  };

  float m = -INFINITY, l = 0.f;  // l: this lane's keys only, until the end
  Acc oa[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) oa[dt] = Acc{};

  const int nkt = cdiv_i(S, kTK);
  fetch(0);
  stash(0);
  __syncthreads();
  for (int kt = 0; kt < nkt; ++kt) {
    const int cur = kt & 1, k0 = kt * kTK;
    const bool more = kt + 1 < nkt;
    if (more) fetch(k0 + kTK);
    if (live) {
      // S^T: lane = query li, registers = keys
      Acc sc[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        sc[j] = Acc{};
#pragma unroll
        for (int ks = 0; ks < NKD; ++ks)
          sc[j] = M::run(
              ld16(&Kl[cur][(j * kR + li) * KP + ks * kKS + kg * 8]), qf[ks],
              sc[j]);
      }
      float tm = -INFINITY;
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < kNR; ++r)
          if (k0 + j * kR + acc_row(r, kg) < S) tm = fmaxf(tm, sc[j][r]);
      tm = fmaxf(tm, __shfl_xor(tm, kR, kWave));
      const float mn = fmaxf(m, tm);
      const float alpha = exp2f((m * scale - mn * scale) * kLog2e);
      m = mn;
      float ps = 0.f;
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < kNR; ++r) {
          const float p =
              k0 + j * kR + acc_row(r, kg) < S
                  ? exp2f((sc[j][r] * scale - mn * scale) * kLog2e)
                  : 0.f;
          sc[j][r] = p;
          ps += p;
        }
      l = l * alpha + ps;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < kNR; ++r) oa[dt][r] *= alpha;
      // O^T += V^T P^T: the accumulator registers, eight at a time, are the
      // B operand; the A operand reads V^T at the keys those registers hold
#pragma unroll
      for (int f = 0; f < NJ * kNR / 8; ++f) {
        short8 pb;
#pragma unroll
        for (int e = 0; e < 8; ++e)
          pb[e] = f32_to_s16<T16>(sc[(8 * f + e) / kNR][(8 * f + e) % kNR]);
        const int key0 = (8 * f) / kNR * kR + acc_row((8 * f) % kNR, kg);
        const int key1 =
            (8 * f + 4) / kNR * kR + acc_row((8 * f + 4) % kNR, kg);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          const short* row = &Vt[cur][(dt * kR + li) * VP];
          oa[dt] = M::run(cat4(row + key0, row + key1), pb, oa[dt]);
        }
      }
    }
    if (more) stash(cur ^ 1);
    __syncthreads();
  }

  if (live) {
    l += __shfl_xor(l, kR, kWave);
    if (qrow < S) {
      const float inv = 1.f / l;
      short* op = reinterpret_cast<short*>(o) + ((long)b * S + qrow) * HD +
                  h * DH;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int g4 = 0; g4 < kNR / 4; ++g4) {
          short4v v;
#pragma unroll
          for (int u = 0; u < 4; ++u)
            v[u] = f32_to_s16<T16>(oa[dt][g4 * 4 + u] * inv);
          *reinterpret_cast<short4v*>(op + dt * kR + 8 * g4 + 4 * kg) = v;
        }
      if (kg == 0) lse[((long)b * H + h) * S + qrow] = m * scale + logf(l);
    }
  }
}

// ---- backward: D and dq -----------------------------------------------------

template <typename T16, int DH>
__global__ __launch_bounds__(256) void flash_bwd_dq_kernel(
    const T16* __restrict__ qkv, const float* __restrict__ lse,
    const T16* __restrict__ dout, T16* __restrict__ dqkv,
    float* __restrict__ dsum, int S, int H, int nqt, float scale) {
  constexpr int NKD = DH / kKS, DT = DH / kR, CV = DH / 8;
  constexpr int KP = DH + 8, VP = kTK + 4;
  constexpr int NLD = kTK * CV / 256;
  constexpr int NJ = kTK / kR;
  using M = AMfma<T16, kR>;
  using Acc = typename M::acc;
  __shared__ __attribute__((aligned(16))) short Kl[2][kTK * KP];
  __shared__ __attribute__((aligned(16))) short Vl[2][kTK * KP];
  __shared__ __attribute__((aligned(16))) short Kt[2][DH * VP];

  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const int li = lane % kR, kg = lane / kR;
  const int bh = blockIdx.x / nqt, qt = blockIdx.x - bh * nqt;
  const int b = bh / H, h = bh - b * H;
  const int HD = H * DH;
  const long rs = 3L * HD;
  const long tok0 = (long)b * S;
  const short* g = reinterpret_cast<const short*>(qkv) + tok0 * rs + h * DH;
  const short* dg = reinterpret_cast<const short*>(dout) + tok0 * HD + h * DH;
  const int qrow = qt * kTQ + w * kR + li;
  const bool live = qt * kTQ + w * kR < S, qok = qrow < S;

  short8 qf[NKD], dof[NKD];
#pragma unroll
  for (int ks = 0; ks < NKD; ++ks) {
    qf[ks] = short8{};
    dof[ks] = short8{};
    if (qok) {
      qf[ks] = ld16(g + qrow * rs + ks * kKS + kg * 8);
      dof[ks] = ld16(dg + (long)qrow * HD + ks * kKS + kg * 8);
    }
  }
  const float L = qok ? lse[((long)b * H + h) * S + qrow] : 0.f;

  short8 kr[NLD], vr[NLD];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int idx = t + i * 256, s = idx / CV, c = idx - s * CV;
      kr[i] = short8{};
      vr[i] = short8{};
      if (k0 + s < S) {
        kr[i] = ld16(g + (k0 + s) * rs + HD + c * 8);
        vr[i] = ld16(g + (k0 + s) * rs + 2 * HD + c * 8);
      }
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int idx = t + i * 256, s = idx / CV, c = idx - s * CV;
      *reinterpret_cast<short8*>(&Kl[buf][s * KP + c * 8]) = kr[i];
      *reinterpret_cast<short8*>(&Vl[buf][s * KP + c * 8]) = vr[i];
#pragma unroll
      for (int e = 0; e < 8; ++e) Kt[buf][(c * 8 + e) * VP + s] = kr[i][e];
    }
  };

  float Dq = 0.f, Zq = 0.f;
  Acc dqt[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) dqt[dt] = Acc{};

  // the key tiles twice over, as one pipeline: iterations [0, nkt) are the
  // D sweep, [nkt, 2 nkt) the dQ sweep
  const int nkt = cdiv_i(S, kTK), nit = 2 * nkt;
  fetch(0);
  stash(0);
  __syncthreads();
  for (int it = 0; it < nit; ++it) {
    const int cur = it & 1;
    const bool second = it >= nkt;
    const int k0 = (second ? it - nkt : it) * kTK;
    const bool more = it + 1 < nit;
    if (more) fetch((it + 1 >= nkt ? it + 1 - nkt : it + 1) * kTK);
    if (live) {
      // S^T and dP^T: lane = query li, registers = keys
      Acc st[NJ], dpt[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        st[j] = Acc{};
        dpt[j] = Acc{};
#pragma unroll
        for (int ks = 0; ks < NKD; ++ks) {
          const int ao = (j * kR + li) * KP + ks * kKS + kg * 8;
          st[j] = M::run(ld16(&Kl[cur][ao]), qf[ks], st[j]);
          dpt[j] = M::run(ld16(&Vl[cur][ao]), dof[ks], dpt[j]);
        }
      }
      if (!second) {
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
          for (int r = 0; r < kNR; ++r)
            if (qok && k0 + j * kR + acc_row(r, kg) < S) {
              const float p = exp2f((st[j][r] * scale - L) * kLog2e);
              Zq += p;
              Dq += p * dpt[j][r];
            }
        if (it == nkt - 1) {
          // D_q = sum_j P dP / sum_j P: see attn.hip on the division
          Dq += __shfl_xor(Dq, kR, kWave);
          Zq += __shfl_xor(Zq, kR, kWave);
          Dq = qok ? Dq / Zq : 0.f;  // rows past S: Zq = 0
          if (qok && kg == 0) dsum[((long)b * H + h) * S + qrow] = Dq;
        }
      } else {
        // dQ^T += K^T dS^T: B = the rounded dS registers, A = K^T
#pragma unroll
        for (int f = 0; f < NJ * kNR / 8; ++f) {
          short8 db;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int j = (8 * f + e) / kNR, r = (8 * f + e) % kNR;
            const bool ok = qok && k0 + j * kR + acc_row(r, kg) < S;
            const float p =
                ok ? exp2f((st[j][r] * scale - L) * kLog2e) : 0.f;
            db[e] = f32_to_s16<T16>(ok ? p * (dpt[j][r] - Dq) : 0.f);
          }
          const int key0 = (8 * f) / kNR * kR + acc_row((8 * f) % kNR, kg);
          const int key1 =
              (8 * f + 4) / kNR * kR + acc_row((8 * f + 4) % kNR, kg);
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) {
            const short* row = &Kt[cur][(dt * kR + li) * VP];
            dqt[dt] = M::run(cat4(row + key0, row + key1), db, dqt[dt]);
          }
        }
      }
    }
    if (more) stash(cur ^ 1);
    __syncthreads();
  }

  if (qok) {
    short* qp = reinterpret_cast<short*>(dqkv) + (tok0 + qrow) * rs + h * DH;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int g4 = 0; g4 < kNR / 4; ++g4) {
        short4v v;
#pragma unroll
        for (int u = 0; u < 4; ++u)
          v[u] = f32_to_s16<T16>(dqt[dt][g4 * 4 + u] * scale);
        *reinterpret_cast<short4v*>(qp + dt * kR + 8 * g4 + 4 * kg) = v;
      }
  }
}

// ---- backward: dk and dv ----------------------------------------------------

template <typename T16, int DH>
__global__ __launch_bounds__(256) void flash_bwd_dkv_kernel(
    const T16* __restrict__ qkv, const float* __restrict__ lse,
    const float* __restrict__ dsum, const T16* __restrict__ dout,
    T16* __restrict__ dqkv, int S, int H, int nkb, float scale) {
  constexpr int NKD = DH / kKS, DT = DH / kR, CV = DH / 8;
  constexpr int QP = DH + 8, TP = kQS + 8;
  using M = AMfma<T16, kR>;
  using Acc = typename M::acc;
  __shared__ __attribute__((aligned(16))) short Ql[2][kQS * QP];
  __shared__ __attribute__((aligned(16))) short dOl[2][kQS * QP];
  __shared__ __attribute__((aligned(16))) short Qt[2][DH * TP];
  __shared__ __attribute__((aligned(16))) short dOt[2][DH * TP];
  __shared__ float Ll[2][kQS], Dl[2][kQS];

  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const int li = lane % kR, kg = lane / kR;
  const int bh = blockIdx.x / nkb, kb = blockIdx.x - bh * nkb;
  const int b = bh / H, h = bh - b * H;
  const int HD = H * DH;
  const long rs = 3L * HD;
  const long tok0 = (long)b * S;
  const short* g = reinterpret_cast<const short*>(qkv) + tok0 * rs + h * DH;
  const short* dg = reinterpret_cast<const short*>(dout) + tok0 * HD + h * DH;
  const float* lg = lse + ((long)b * H + h) * S;
  const float* sg = dsum + ((long)b * H + h) * S;
  const int key = kb * kTQ + w * kR + li;
  const bool live = kb * kTQ + w * kR < S, kok = key < S;

  // the wave's keys: K and V fragments in registers for the whole kernel
  short8 kf[NKD], vf[NKD];
  Acc dkt[DT], dvt[DT];
#pragma unroll
  for (int ks = 0; ks < NKD; ++ks) {
    kf[ks] = short8{};
    vf[ks] = short8{};
    if (kok) {
      kf[ks] = ld16(g + key * rs + HD + ks * kKS + kg * 8);
      vf[ks] = ld16(g + key * rs + 2 * HD + ks * kKS + kg * 8);
    }
  }
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) {
    dkt[dt] = Acc{};
    dvt[dt] = Acc{};
  }

  // one 16-byte chunk of Q and of dO per staging thread and step
  const bool stager = t < kQS * CV;
  const int srow = t / CV, sc = t - srow * CV;
  short8 qr = {}, dr = {};
  float lr = 0.f, sr = 0.f;
  auto fetch = [&](int q0) {
    if (stager) {
      const int qrow = q0 + srow;
      qr = short8{};
      dr = short8{};
      lr = sr = 0.f;
      if (qrow < S) {
        qr = ld16(g + qrow * rs + sc * 8);
        dr = ld16(dg + (long)qrow * HD + sc * 8);
        if (sc == 0) {
          lr = lg[qrow];
          sr = sg[qrow];
        }
      }
    }
  };
  auto stash = [&](int buf) {
    if (stager) {
      *reinterpret_cast<short8*>(&Ql[buf][srow * QP + sc * 8]) = qr;
      *reinterpret_cast<short8*>(&dOl[buf][srow * QP + sc * 8]) = dr;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        Qt[buf][(sc * 8 + e) * TP + srow] = qr[e];
        dOt[buf][(sc * 8 + e) * TP + srow] = dr[e];
      }
      if (sc == 0) {
        Ll[buf][srow] = lr;
        Dl[buf][srow] = sr;
      }
    }
  };

  const int nqs = cdiv_i(S, kQS);
  fetch(0);
  stash(0);
  __syncthreads();
  for (int qs = 0; qs < nqs; ++qs) {
    const int cur = qs & 1, q0 = qs * kQS;
    const bool more = qs + 1 < nqs;
    if (more) fetch(q0 + kQS);
    if (live) {
      // S = Q K^T and dP = dO V^T: lane = key li, registers = queries
      Acc st = {}, dp = {};
#pragma unroll
      for (int ks = 0; ks < NKD; ++ks) {
        const int ao = li * QP + ks * kKS + kg * 8;
        st = M::run(ld16(&Ql[cur][ao]), kf[ks], st);
        dp = M::run(ld16(&dOl[cur][ao]), vf[ks], dp);
      }
      // P and dS, rounded once: the B operands of the two products below
      short8 pb[kNR / 8], db[kNR / 8];
#pragma unroll
      for (int r = 0; r < kNR; ++r) {
        const int ql = acc_row(r, kg);
        const bool ok = kok && q0 + ql < S;
        const float p =
            ok ? exp2f((st[r] * scale - Ll[cur][ql]) * kLog2e) : 0.f;
        const float ds = ok ? p * (dp[r] - Dl[cur][ql]) : 0.f;
        pb[r / 8][r % 8] = f32_to_s16<T16>(p);
        db[r / 8][r % 8] = f32_to_s16<T16>(ds);
      }
      // dV^T += dO^T P, dK^T += Q^T dS: the A operand reads dO^T and Q^T at
      // the queries those registers hold
#pragma unroll
      for (int f = 0; f < kNR / 8; ++f) {
        const int qa = acc_row(8 * f, kg), qb = acc_row(8 * f + 4, kg);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          const int ao = (dt * kR + li) * TP;
          dvt[dt] = M::run(cat4(&dOt[cur][ao + qa], &dOt[cur][ao + qb]),
                           pb[f], dvt[dt]);
          dkt[dt] = M::run(cat4(&Qt[cur][ao + qa], &Qt[cur][ao + qb]), db[f],
                           dkt[dt]);
        }
      }
    }
    if (more) stash(cur ^ 1);
    __syncthreads();
  }

  if (kok) {
    short* kp = reinterpret_cast<short*>(dqkv) + (tok0 + key) * rs + h * DH +
                HD;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int g4 = 0; g4 < kNR / 4; ++g4) {
        short4v vk, vv;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          vk[u] = f32_to_s16<T16>(dkt[dt][g4 * 4 + u] * scale);
          vv[u] = f32_to_s16<T16>(dvt[dt][g4 * 4 + u]);
        }
        const int d = dt * kR + 8 * g4 + 4 * kg;
        *reinterpret_cast<short4v*>(kp + d) = vk;
        *reinterpret_cast<short4v*>(kp + HD + d) = vv;
      }
  }
}

#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif

// ---- host -------------------------------------------------------------------

struct FlashDims {
  int B, S, H, dh;
  int nt;         // 128-token tiles of a head (queries or keys)
  unsigned grid;  // B * H * nt, the tile fastest
};

FlashDims flash_dims(const at::Tensor& qkv) {
  CHECK_GPU(qkv);
  CHECK_CONTIG(qkv);
  CHECK_16BIT(qkv);
  TORCH_CHECK(qkv.dim() == 5 && qkv.size(2) == 3,
              "flash attention: qkv must be [B,S,3,H,dh]");
  const long B = qkv.size(0), S = qkv.size(1), H = qkv.size(3),
             dh = qkv.size(4);
  TORCH_CHECK(dh == 32 || dh == 64, "flash attention: head width=", dh,
              " must be 32 or 64");
  TORCH_CHECK(S >= 1 && S <= 4096, "flash attention: sequence length=", S,
              " must be in [1, 4096]");
  const long nt = cdiv_l(S, kTQ);
  TORCH_CHECK(B >= 1 && H >= 1 && B * H * nt < (1L << 31) &&
                  H * dh < (1L << 20),
              "flash attention: batch or head count too large");
  return FlashDims{(int)B, (int)S, (int)H, (int)dh, (int)nt,
                   (unsigned)(B * H * nt)};
}

}  // namespace

// returns {o[B,S,H*dh], lse[B,H,S]}
std::vector<at::Tensor> flash_attn_fwd(at::Tensor qkv, double scale) {
  const FlashDims d = flash_dims(qkv);
  auto o = at::empty({d.B, d.S, (long)d.H * d.dh}, qkv.options());
  auto lse = at::empty({d.B, d.H, d.S}, qkv.options().dtype(at::kFloat));
  DISPATCH_16(qkv, T16, {
    pick<32, 64>(d.dh, [&](auto DH) {
      launch256((flash_fwd_kernel<T16, decltype(DH)::value>), dim3(d.grid), 0,
                (const T16*)qkv.data_ptr(), (T16*)o.data_ptr(),
                lse.data_ptr<float>(), d.S, d.H, d.nt, (float)scale);
    });
  });
  return {o, lse};
}

// returns dqkv[B,S,3,H,dh], every element written
at::Tensor flash_attn_bwd(at::Tensor qkv, at::Tensor lse, at::Tensor dout,
                          double scale) {
  const FlashDims d = flash_dims(qkv);
  TORCH_CHECK(dout.is_cuda() && dout.is_contiguous() &&
                  dout.scalar_type() == qkv.scalar_type() && dout.dim() == 3 &&
                  dout.size(0) == d.B && dout.size(1) == d.S &&
                  dout.size(2) == (long)d.H * d.dh,
              "flash attention: do must be contiguous [B,S,H*dh] of qkv's "
              "dtype");
  TORCH_CHECK(lse.is_cuda() && lse.is_contiguous() &&
                  lse.scalar_type() == at::kFloat &&
                  lse.numel() == (long)d.B * d.H * d.S,
              "flash attention: lse must be fp32 [B,H,S]");
  auto dqkv = at::empty_like(qkv);
  auto dsum = at::empty_like(lse);  // D[B,H,S], dq kernel -> dkv kernel
  DISPATCH_16(qkv, T16, {
    pick<32, 64>(d.dh, [&](auto DH) {
      launch256((flash_bwd_dq_kernel<T16, decltype(DH)::value>), dim3(d.grid),
                0, (const T16*)qkv.data_ptr(), lse.data_ptr<float>(),
                (const T16*)dout.data_ptr(), (T16*)dqkv.data_ptr(),
                dsum.data_ptr<float>(), d.S, d.H, d.nt, (float)scale);
      launch256((flash_bwd_dkv_kernel<T16, decltype(DH)::value>),
                dim3(d.grid), 0, (const T16*)qkv.data_ptr(),
                lse.data_ptr<float>(), dsum.data_ptr<float>(),
                (const T16*)dout.data_ptr(), (T16*)dqkv.data_ptr(), d.S, d.H,
                d.nt, (float)scale);
    });
  });
  return dqkv;
}
