// Transformer MLP (ops.mlp):  z = x w1^T + b1;  h = act(z);  y = h w2^T + b2
// with act = exact GELU or ReLU, forward and backward in six GEMM launches
// of two kernels. bf16 / fp16 operands, fp32 accumulation on
// v_mfma_f32_32x32x16, gfx950 only.
//
// mlp_nt_kernel: out[M,N] = A[M,K] B[N,K]^T with the MLP's epilogues.
//   128x128 block tile, four waves of 64x64 (2x2 MFMA tiles, 64 accumulator
//   registers): a 16-wide k-slice is two A and two B fragment reads for four
//   MFMAs. The LDS tiles [row][BK+8] are double-buffered: the next stage's
//   global loads are issued before the current stage's MFMAs, written to the
//   other buffer after them, and one barrier closes the k-step. BK is 32
//   (40 KiB) or 64 (72 KiB of dynamic LDS); profiles/r19_mlp.md has the A/B.
//   The accumulators leave as whole rows in 16-byte stores through the
//   wave-private staging of conv_epilogue.h (EpiTile<2>, one 32-row half of
//   the wave's tile per pass); the fetch and flush here add the N-tail
//   guard that the conv kernels do not need. Epilogues, per instantiation:
//     EPI_BIAS        v + b                                   (fc2)
//     EPI_BIAS_RELU   h = relu(v + b)                         (fc1)
//     EPI_BIAS_GELU   z = v + b and h = gelu(z), both stored  (fc1)
//     EPI_PLAIN       v                                       (dx = dz w1)
//     EPI_DRELU       v * (h > 0), h read as a row tile       (dz = dh .)
//     EPI_DGELU       v * gelu'(z), z read as a row tile      (dz = dh .)
//   erff runs once per output element, in the epilogue only; dh is never
//   stored.
//
// mlp_tn_kernel: dw[N,K] = dy[M,N]^T x[M,K] and db[N] = column sums of dy,
//   straight from the row-major operands. Per 64-row m-step, waves 0-1 read
//   the dy tile and waves 2-3 the x tile as 8x8 patches (eight 16-byte loads
//   along N or K), transpose the patch in registers and write eight 16-byte
//   LDS rows [n][m]: an MFMA fragment is then one 16-byte read. Columns are
//   rotated by the row's 8-group (the k-minor swizzle of the conv wgrads) so
//   the transposed writes of a patch column spread over the banks. The next
//   step's loads ride under the MFMAs. M is split over blockIdx.z into
//   chunks of a multiple of 64 rows; fp32 partials [chunks,N,K] and
//   [chunks,N] are folded by fold_rows in a fixed order (no atomics). The
//   blocks of k-tile column 0 sum the dy patches they stage for db.
#include "common.h"
#include "conv_epilogue.h"

typedef __attribute__((ext_vector_type(8))) _Float16 half8_m;
typedef __attribute__((ext_vector_type(16))) float f32x16_m;

namespace {

constexpr int TB = 128;  // block tile edge of both kernels
enum { EPI_BIAS, EPI_BIAS_RELU, EPI_BIAS_GELU, EPI_PLAIN, EPI_DRELU,
       EPI_DGELU };
constexpr int ACT_RELU = 1, ACT_GELU = 2;

template <typename T16>
struct MMfma {};
template <>
struct MMfma<__hip_bfloat16> {
  static DEV_INLINE f32x16_m run(short8 a, short8 b, f32x16_m c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
};
template <>
struct MMfma<__half> {
  static DEV_INLINE f32x16_m run(short8 a, short8 b, f32x16_m c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16((half8_m)a, (half8_m)b, c,
                                                  0, 0, 0);
  }
};

// exact GELU, 0.5 v (1 + erf(v / sqrt 2)), and its derivative
// Phi(z) + z phi(z)
DEV_INLINE float gelu_f(float v) {
  return 0.5f * v * (1.f + erff(v * 0.70710678118654752f));
}
DEV_INLINE float dgelu_f(float z) {
  return 0.5f * (1.f + erff(z * 0.70710678118654752f)) +
         z * 0.39894228040143268f * expf(-0.5f * z * z);
}

using E2 = EpiTile<2>;

// epi_fetch / epi_flush of conv_epilogue.h with a column bound: only the
// 16-byte pieces that start below `ncols` move (N % 8 == 0)
template <typename T16>
DEV_INLINE void tile_fetch(short* wl, const T16* __restrict__ g, int lane,
                           const long (&roff)[E2::NIT], int ncols) {
  const int c = (lane % E2::LPR) * 8;
  short8 v[E2::NIT];
#pragma unroll
  for (int it = 0; it < E2::NIT; ++it)
    v[it] = (roff[it] >= 0 && c < ncols)
                ? *reinterpret_cast<const short8*>(g + roff[it] + c)
                : short8{};
#pragma unroll
  for (int it = 0; it < E2::NIT; ++it)
    *reinterpret_cast<short8*>(wl + epi_io_row<2>(it, lane) * E2::RS + c) =
        v[it];
}

template <typename T16>
DEV_INLINE void tile_flush(const short* wl, T16* __restrict__ g, int lane,
                           const long (&roff)[E2::NIT], int ncols) {
  const int c = (lane % E2::LPR) * 8;
#pragma unroll
  for (int it = 0; it < E2::NIT; ++it) {
    const short8 v = *reinterpret_cast<const short8*>(
        wl + epi_io_row<2>(it, lane) * E2::RS + c);
    if (roff[it] >= 0 && c < ncols)
      *reinterpret_cast<short8*>(g + roff[it] + c) = v;
  }
}

template <typename T16, int BK, int EPI>
__global__ __launch_bounds__(256, 2) void mlp_nt_kernel(
    const T16* __restrict__ A,       // [M, K]
    const T16* __restrict__ B,       // [N, K]
    const float* __restrict__ bias,  // [N] (EPI_BIAS*)
    const T16* __restrict__ side,    // [M, N]: h (EPI_DRELU) or z (EPI_DGELU)
    T16* __restrict__ out,           // [M, N]
    T16* __restrict__ out2,          // [M, N]: z (EPI_BIAS_GELU)
    const int M, const int N, const int K) {
  extern __shared__ __attribute__((aligned(16))) short lds[];
  constexpr int LDK = BK + 8;          // +16 B pad: fragment reads off banks
  constexpr int STAGE = 2 * TB * LDK;  // A tile, then B tile
  constexpr int VPR = BK / 8;          // 16-byte vectors per tile row
  constexpr int RPP = 256 / VPR;       // tile rows one pass of the block covers
  constexpr int NP = TB / RPP;         // passes per tile
  static_assert(2 * STAGE * 2 >= E2::BYTES, "epilogue staging fits");

  const int tid = threadIdx.x;
  const long bm0 = (long)blockIdx.x * TB;
  const int n0 = blockIdx.y * TB;
  const int sr = tid / VPR;
  const int sc = (tid % VPR) * 8;

  const int wave = tid >> 6, lane = tid & 63;
  const int li = lane & 31, kh = lane >> 5;
  const int wm = (wave & 1) * 64, wn = (wave >> 1) * 64;

  f32x16_m acc[2][2] = {};
  const int ksteps = (K + BK - 1) / BK;

  short8 ra[NP], rb[NP];
  auto load_step = [&](int j) {
    const int k = j * BK + sc;
    const bool k_ok = k < K;  // K % 8 == 0: a vector is all in or all out
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const long m = bm0 + sr + p * RPP;
      const int n = n0 + sr + p * RPP;
      ra[p] = (k_ok && m < M)
                  ? *reinterpret_cast<const short8*>(A + m * K + k)
                  : short8{};
      rb[p] = (k_ok && n < N)
                  ? *reinterpret_cast<const short8*>(B + (long)n * K + k)
                  : short8{};
    }
  };
  // B row n of a wave's 64 goes to LDS row epi_brow<2>: accumulator tile t of
  // lane li is then channel li*2 + t (conv_epilogue.h)
  auto stage = [&](int s) {
    short* base = lds + s * STAGE;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int r = sr + p * RPP;
      *reinterpret_cast<short8*>(base + r * LDK + sc) = ra[p];
      const int br = (r & 64) + epi_brow<2>(r & 63);
      *reinterpret_cast<short8*>(base + (TB + br) * LDK + sc) = rb[p];
    }
  };

  load_step(0);
  stage(0);
  __syncthreads();
  for (int j = 0; j < ksteps; ++j) {
    const bool more = j + 1 < ksteps;
    if (more) load_step(j + 1);  // in flight during this stage's MFMAs
    const short* la = lds + (j & 1) * STAGE + (wm + li) * LDK + kh * 8;
    const short* lb = lds + (j & 1) * STAGE + (TB + wn + li) * LDK + kh * 8;
#pragma unroll
    for (int kk = 0; kk < BK; kk += 16) {
      const short8 a0 = *reinterpret_cast<const short8*>(la + kk);
      const short8 a1 = *reinterpret_cast<const short8*>(la + 32 * LDK + kk);
      const short8 b0 = *reinterpret_cast<const short8*>(lb + kk);
      const short8 b1 = *reinterpret_cast<const short8*>(lb + 32 * LDK + kk);
      acc[0][0] = MMfma<T16>::run(a0, b0, acc[0][0]);
      acc[0][1] = MMfma<T16>::run(a0, b1, acc[0][1]);
      acc[1][0] = MMfma<T16>::run(a1, b0, acc[1][0]);
      acc[1][1] = MMfma<T16>::run(a1, b1, acc[1][1]);
    }
    // the other buffer was last read before the previous barrier
    if (more) stage((j + 1) & 1);
    __syncthreads();
  }

  // epilogue: every wave is past the last barrier, the tiles are dead
  short* wl = lds + wave * E2::WAVE;
  const int nw = n0 + wn;       // first channel of the wave's tile
  const int ncols = N - nw;     // <= 0: the whole tile is N tail
  const int ch = nw + li * 2;   // this lane's two channels: ch, ch + 1
  float bv[2] = {0.f, 0.f};
  if (EPI == EPI_BIAS || EPI == EPI_BIAS_RELU || EPI == EPI_BIAS_GELU) {
    if (ch < N) {  // N is even: ch + 1 < N too
      bv[0] = bias[ch];
      bv[1] = bias[ch + 1];
    }
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    long roff[E2::NIT];
#pragma unroll
    for (int it = 0; it < E2::NIT; ++it) {
      const long m = bm0 + wm + i * 32 + epi_io_row<2>(it, lane);
      roff[it] = m < M ? m * N + nw : -1;
    }
    if (EPI == EPI_DRELU || EPI == EPI_DGELU) {
      tile_fetch<T16>(wl, side, lane, roff, ncols);
      epi_wave_sync();
    }
    short2v second[16];  // z of EPI_BIAS_GELU, stored after h
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int row = epi_acc_row(reg, kh);
      float v[2] = {acc[i][0][reg] + bv[0], acc[i][1][reg] + bv[1]};
      if (EPI == EPI_BIAS_RELU) {
        v[0] = relu_f(v[0]);
        v[1] = relu_f(v[1]);
      } else if (EPI == EPI_BIAS_GELU) {
        second[reg] = short2v{f32_to_s16<T16>(v[0]), f32_to_s16<T16>(v[1])};
        v[0] = gelu_f(v[0]);
        v[1] = gelu_f(v[1]);
      } else if (EPI == EPI_DRELU) {
        const short2v s = epi_get<2>(wl, row, li);
        v[0] = s16_to_f32<T16>(s[0]) > 0.f ? v[0] : 0.f;
        v[1] = s16_to_f32<T16>(s[1]) > 0.f ? v[1] : 0.f;
      } else if (EPI == EPI_DGELU) {
        const short2v s = epi_get<2>(wl, row, li);
        v[0] *= dgelu_f(s16_to_f32<T16>(s[0]));
        v[1] *= dgelu_f(s16_to_f32<T16>(s[1]));
      }
      epi_put<2>(wl, row, li,
                 short2v{f32_to_s16<T16>(v[0]), f32_to_s16<T16>(v[1])});
    }
    epi_wave_sync();
    tile_flush<T16>(wl, out, lane, roff, ncols);
    epi_wave_sync();
    if (EPI == EPI_BIAS_GELU) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg)
        epi_put<2>(wl, epi_acc_row(reg, kh), li, second[reg]);
      epi_wave_sync();
      tile_flush<T16>(wl, out2, lane, roff, ncols);
      epi_wave_sync();
    }
  }
}

constexpr int TM = 64;   // m rows per step of the TN kernel
constexpr int LDM = 72;  // m-minor LDS row (+16 B: alignment and banks)

template <typename T16>
__global__ __launch_bounds__(256, 2) void mlp_tn_kernel(
    const T16* __restrict__ dy,    // [M, N]
    const T16* __restrict__ x,     // [M, K]
    float* __restrict__ dw_part,   // [chunks, N, K]
    float* __restrict__ db_part,   // [chunks, N]
    const int M, const int N, const int K, const int m_per_chunk) {
  __shared__ __attribute__((aligned(16))) short lds[2 * TB * LDM];
  const int tid = threadIdx.x;
  const int k0 = blockIdx.x * TB, n0 = blockIdx.y * TB;
  const int m_begin = blockIdx.z * m_per_chunk;
  const int m_end = min(M, m_begin + m_per_chunk);

  // staging: waves 0-1 take dy, waves 2-3 take x; a thread owns the 8x8
  // patch (m-group pm, column-group pc). Of a 16-lane group, 8 lanes cover
  // 128 contiguous bytes of one row and the other 8 the row 8 below.
  const bool is_x = tid >= 128;
  const int p = tid & 127;
  const int pc = (p & 7) | ((p >> 1) & 8);
  const int pm = ((p >> 3) & 1) | ((p >> 4) & 6);
  const T16* src = is_x ? x : dy;
  const int ld = is_x ? K : N;
  const int c0 = (is_x ? k0 : n0) + pc * 8;
  const bool c_ok = c0 < ld;  // ld % 8 == 0: a vector is all in or all out
  // transposed rows pc*8 .. +7, m-columns rotated by the row's 8-group
  short* wbase =
      lds + (is_x ? TB * LDM : 0) + pc * 8 * LDM + ((pm + pc) & 7) * 8;
  const bool do_db = !is_x && blockIdx.x == 0;
  float csum[8] = {};

  short8 v[8];
  auto load_step = [&](int m0) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int m = m0 + pm * 8 + r;
      v[r] = (c_ok && m < m_end)
                 ? *reinterpret_cast<const short8*>(src + (long)m * ld + c0)
                 : short8{};
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const short8 t = {v[0][e], v[1][e], v[2][e], v[3][e],
                        v[4][e], v[5][e], v[6][e], v[7][e]};
      *reinterpret_cast<short8*>(wbase + e * LDM) = t;
    }
    if (do_db) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < 8; ++r) s += s16_to_f32<T16>(v[r][e]);
        csum[e] += s;
      }
    }
  };

  const int wave = tid >> 6, lane = tid & 63;
  const int li = lane & 31, kh = lane >> 5;
  const int wn = (wave & 1) * 64, wk = (wave >> 1) * 64;
  f32x16_m acc[2][2] = {};

  load_step(m_begin);
  for (int m0 = m_begin; m0 < m_end; m0 += TM) {
    __syncthreads();  // the previous MFMA phase is done reading
    stage();
    __syncthreads();
    if (m0 + TM < m_end) load_step(m0 + TM);  // rides under the MFMAs
    const short* la = lds + (wn + li) * LDM;
    const short* lb = lds + (TB + wk + li) * LDM;
    // the rotation is (row & 56): li's for rows 0-31 (wn, wk are multiples
    // of 64), 32 more for rows 32-63
    const int rot = li & 56;
#pragma unroll
    for (int kk = 0; kk < TM; kk += 16) {
      const int col = (kk + kh * 8 + rot) & 63, col1 = col ^ 32;
      const short8 a0 = *reinterpret_cast<const short8*>(la + col);
      const short8 a1 = *reinterpret_cast<const short8*>(la + 32 * LDM + col1);
      const short8 b0 = *reinterpret_cast<const short8*>(lb + col);
      const short8 b1 = *reinterpret_cast<const short8*>(lb + 32 * LDM + col1);
      acc[0][0] = MMfma<T16>::run(a0, b0, acc[0][0]);
      acc[0][1] = MMfma<T16>::run(a0, b1, acc[0][1]);
      acc[1][0] = MMfma<T16>::run(a1, b0, acc[1][0]);
      acc[1][1] = MMfma<T16>::run(a1, b1, acc[1][1]);
    }
  }

  // fp32 partial tile: a register is one output row, 128 bytes per 32 lanes
  float* part = dw_part + (long)blockIdx.z * N * K;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int k = k0 + wk + t * 32 + li;
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int n = n0 + wn + i * 32 + epi_acc_row(reg, kh);
        if (n < N && k < K) part[(long)n * K + k] = acc[i][t][reg];
      }
    }

  if (blockIdx.x == 0) {  // db: the 8 m-groups of a column meet in LDS
    float* red = reinterpret_cast<float*>(lds);
    __syncthreads();
    if (!is_x) {
#pragma unroll
      for (int e = 0; e < 8; ++e) red[pm * TB + pc * 8 + e] = csum[e];
    }
    __syncthreads();
    if (tid < TB && n0 + tid < N) {
      float s = red[tid];
#pragma unroll
      for (int g = 1; g < 8; ++g) s += red[g * TB + tid];
      db_part[(long)blockIdx.z * N + n0 + tid] = s;
    }
  }
}

// bk: 0 = the rule (32), or 32 / 64 (benchmarks/mlp_bench.py's A/B)
template <int EPI>
void launch_nt(const at::Tensor& A, const at::Tensor& B, const float* bias,
               const void* side, void* out, void* out2, long bk) {
  const int M = A.size(0), K = A.size(1), N = B.size(0);
  TORCH_CHECK(B.size(1) == K, "mlp: inner dimensions differ");
  dim3 grid((unsigned)cdiv_l(M, TB), (unsigned)cdiv_l(N, TB));
  DISPATCH_16(A, T16, {
    pick<32, 64>(bk == 0 ? 32 : (int)bk, [&](auto BK) {
      auto kern = mlp_nt_kernel<T16, BK, EPI>;
      constexpr size_t bytes = 2 * 2 * TB * (BK + 8) * 2;
      if (bytes > 64 * 1024) {  // above the static limit: raise it once
        static const hipError_t raised = hipFuncSetAttribute(
            reinterpret_cast<const void*>(kern),
            hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        TORCH_CHECK(raised == hipSuccess, "mlp: cannot raise the LDS limit");
      }
      launch256(kern, grid, bytes, (const T16*)A.data_ptr(),
                (const T16*)B.data_ptr(), bias, (const T16*)side, (T16*)out,
                (T16*)out2, M, N, K);
    });
  });
}

// dw[N,K], db[N] (fp32) from dy[M,N] and x[M,K]
void launch_tn(const at::Tensor& dy, const at::Tensor& x, at::Tensor& dw,
               at::Tensor& db) {
  const int M = dy.size(0), N = dy.size(1), K = x.size(1);
  const long tiles = cdiv_l(N, TB) * cdiv_l(K, TB);
  const long cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  // about two blocks per CU, chunks of whole m-steps
  const SplitPlan plan = split_plan(M, cdiv_l(2 * cus, tiles), TM);
  auto f32 = dy.options().dtype(at::kFloat);
  at::Tensor dwp = plan.n == 1 ? dw : at::empty({plan.n, N, K}, f32);
  at::Tensor dbp = plan.n == 1 ? db : at::empty({plan.n, N}, f32);
  dim3 grid((unsigned)cdiv_l(K, TB), (unsigned)cdiv_l(N, TB),
            (unsigned)plan.n);
  DISPATCH_16(dy, T16, {
    launch256(mlp_tn_kernel<T16>, grid, 0, (const T16*)dy.data_ptr(),
              (const T16*)x.data_ptr(), dwp.data_ptr<float>(),
              dbp.data_ptr<float>(), M, N, K, (int)plan.per);
  });
  if (plan.n > 1) {
    fold_rows(dwp, dw, (long)N * K, plan.n);
    fold_rows(dbp, db, N, plan.n);
  }
}

void check_mlp(const at::Tensor& x, long D, long F, long act) {
  CHECK_GPU(x);
  CHECK_CONTIG(x);
  CHECK_16BIT(x);
  TORCH_CHECK(x.dim() == 2 && x.size(0) >= 1 && x.size(0) < (1L << 31) / TB,
              "mlp: x must be [M, D] with 1 <= M < 2^24");
  TORCH_CHECK(D >= 8 && D % 8 == 0 && F >= 8 && F % 8 == 0,
              "mlp: D and F must be multiples of 8");
  TORCH_CHECK(act == ACT_RELU || act == ACT_GELU, "mlp: unknown activation");
}

}  // namespace

// x [M,D], w1 [F,D], w2 [D,F] 16-bit; b1 [F], b2 [D] fp32.
// Returns {y, h, z}; z is empty for ReLU.
std::vector<at::Tensor> mlp_fwd(at::Tensor x, at::Tensor w1, at::Tensor b1,
                                at::Tensor w2, at::Tensor b2, long act,
                                long bk) {
  const long M = x.size(0), D = w1.size(1), F = w1.size(0);
  check_mlp(x, D, F, act);
  CHECK_CONTIG(w1);
  CHECK_CONTIG(w2);
  TORCH_CHECK(x.size(1) == D && w2.size(0) == D && w2.size(1) == F &&
                  b1.numel() == F && b2.numel() == D,
              "mlp_fwd: parameter shapes do not fit x");
  TORCH_CHECK(w1.scalar_type() == x.scalar_type() &&
                  w2.scalar_type() == x.scalar_type() &&
                  b1.scalar_type() == at::kFloat &&
                  b2.scalar_type() == at::kFloat,
              "mlp_fwd: weights in x's dtype, biases in fp32");
  auto h = at::empty({M, F}, x.options());
  auto z = at::empty({act == ACT_GELU ? M : 0, F}, x.options());
  auto y = at::empty({M, D}, x.options());
  if (act == ACT_GELU)
    launch_nt<EPI_BIAS_GELU>(x, w1, b1.data_ptr<float>(), nullptr,
                             h.data_ptr(), z.data_ptr(), bk);
  else
    launch_nt<EPI_BIAS_RELU>(x, w1, b1.data_ptr<float>(), nullptr,
                             h.data_ptr(), nullptr, bk);
  launch_nt<EPI_BIAS>(h, w2, b2.data_ptr<float>(), nullptr, y.data_ptr(),
                      nullptr, bk);
  return {y, h, z};
}

// dy [M,D]; x, h, z of the forward; w1t [D,F], w2t [F,D] the cached
// transposes. Returns {dx (empty unless want_dx), dw1, db1, dw2, db2}.
std::vector<at::Tensor> mlp_bwd(at::Tensor dy, at::Tensor x, at::Tensor h,
                                at::Tensor z, at::Tensor w1t, at::Tensor w2t,
                                long act, bool want_dx, long bk) {
  const long M = x.size(0), D = x.size(1), F = h.size(1);
  check_mlp(dy, D, F, act);
  CHECK_CONTIG(x);
  CHECK_CONTIG(h);
  CHECK_CONTIG(z);
  CHECK_CONTIG(w1t);
  CHECK_CONTIG(w2t);
  const at::Tensor& side = act == ACT_GELU ? z : h;
  TORCH_CHECK(dy.size(0) == M && dy.size(1) == D && h.size(0) == M &&
                  side.size(0) == M && side.size(1) == F &&
                  w1t.size(0) == D && w1t.size(1) == F && w2t.size(0) == F &&
                  w2t.size(1) == D,
              "mlp_bwd: shapes do not fit");
  TORCH_CHECK(x.scalar_type() == dy.scalar_type() &&
                  h.scalar_type() == dy.scalar_type() &&
                  side.scalar_type() == dy.scalar_type() &&
                  w1t.scalar_type() == dy.scalar_type() &&
                  w2t.scalar_type() == dy.scalar_type(),
              "mlp_bwd: one 16-bit dtype throughout");
  auto f32 = dy.options().dtype(at::kFloat);
  auto dw2 = at::empty({D, F}, f32), db2 = at::empty({D}, f32);
  auto dw1 = at::empty({F, D}, f32), db1 = at::empty({F}, f32);
  launch_tn(dy, h, dw2, db2);
  auto dz = at::empty({M, F}, dy.options());
  if (act == ACT_GELU)
    launch_nt<EPI_DGELU>(dy, w2t, nullptr, z.data_ptr(), dz.data_ptr(),
                         nullptr, bk);
  else
    launch_nt<EPI_DRELU>(dy, w2t, nullptr, h.data_ptr(), dz.data_ptr(),
                         nullptr, bk);
  launch_tn(dz, x, dw1, db1);
  auto dx = at::empty({want_dx ? M : 0, D}, dy.options());
  if (want_dx)
    launch_nt<EPI_PLAIN>(dz, w1t, nullptr, nullptr, dx.data_ptr(), nullptr,
                         bk);
  return {dx, dw1, db1, dw2, db2};
}
