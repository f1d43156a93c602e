// Device-resident batch builder: gather by sampler index from the uint8 NHWC
// dataset in HBM, zero-pad + random-crop, horizontal flip, normalize, convert
// to the 16-bit compute dtype and write NHWC — one pass, no host work.
//
// The random draws are counter-based and keyed on the DATASET index (not the
// batch position), so a sample's augmentation in an epoch is identical at
// any batch size, world size or rank. mi355x.data.augment_params is the same
// function in torch integer ops (the CPU path and the tests' oracle).
//
// Each lane owns 8 consecutive output elements and stores them as one 16 B
// short8; the source reads are byte gathers (a flipped or shifted row of a
// 3 KB sample) served by L2. Measured 46 us at batch 8192 x 32x32x3, about
// 1.65 TB/s: bound by issuing the gathers, not by bandwidth, and 0.08 % of
// the ResNet-18 step (profiles/r04_device_loader.md).
#include "common.h"

#include <climits>
#include <tuple>

// The normalize must round twice (mul, then add) to equal the CPU path bit
// for bit. hipcc's default -ffp-contract=fast fuses a*b+c, and it fuses
// __fadd_rn(__fmul_rn(a,b),c) just the same (one v_fmac_f32 in the ISA: the
// header's wrappers are plain * and + compiled under the default mode). So
// contraction is off for this file and the normalize is a plain mul and add.
#pragma clang fp contract(off)

namespace {

__host__ __device__ inline unsigned mix32(unsigned h) {
  h ^= h >> 16;
  h *= 0x7feb352du;
  h ^= h >> 15;
  h *= 0x846ca68bu;
  h ^= h >> 16;
  return h;
}

// crop offset and flip of dataset sample i, packed by aug_draw
struct Draw {
  int oy, ox;  // dy - pad, dx - pad
  bool f;
};

DEV_INLINE Draw aug_draw(unsigned i, unsigned key, unsigned span, int pad,
                         bool flip) {
  const unsigned h = mix32(i ^ key);
  const unsigned h2 = mix32(h + 0x9E3779B9u);
  Draw d;
  d.oy = (int)(((h & 0xffffu) * span) >> 16) - pad;
  d.ox = (int)(((h >> 16) * span) >> 16) - pad;
  d.f = flip && (h2 & 1u);
  return d;
}

template <typename T16>
__global__ void gather_augment_kernel(
    const unsigned char* __restrict__ data, const long* __restrict__ targets,
    const int* __restrict__ indices, const float* __restrict__ scale,
    const float* __restrict__ shift, T16* __restrict__ x,
    long* __restrict__ y, int N, int B, int H, int W, int C, int pad,
    bool flip, unsigned key) {
  const int HWC = H * W * C;
  const long total = (long)B * HWC;
  const unsigned span = 2u * (unsigned)pad + 1u;
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long nthr = (long)gridDim.x * blockDim.x;

  for (long b = tid; b < B; b += nthr) {
    const int i = indices[b];
    // an index outside the dataset reads nothing: label -1 (the loss
    // kernel poisons on it) and, below, an all-padding image
    y[b] = (unsigned)i < (unsigned)N ? targets[i] : -1;
  }

  float sc[4], sf[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    sc[c] = c < C ? scale[c] : 0.f;
    sf[c] = c < C ? shift[c] : 0.f;
  }

  for (long e0 = tid * 8; e0 < total; e0 += nthr * 8) {
    // (b,h,w,c) of the first element; the other 7 follow by carry
    long b = e0 / HWC;
    int r = (int)(e0 - b * HWC);
    int h = r / (W * C);
    r -= h * (W * C);
    int w = r / C;
    int c = r - w * C;
    const int cnt = (int)(total - e0 < 8 ? total - e0 : 8);

    int i = indices[b];
    bool ok = (unsigned)i < (unsigned)N;
    Draw d = aug_draw((unsigned)i, key, span, pad, flip);
    short8 o;
    // every lane builds all 8 (no per-element tail test: past the end the
    // walk stays on the last sample and the values are not stored)
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int sh = h + d.oy;
      const int sw = (d.f ? W - 1 - w : w) + d.ox;
      // branch-free: always load from a clamped in-range address and
      // select, so the 8 byte gathers of a lane are in flight together
      const bool in = ok && sh >= 0 && sh < H && sw >= 0 && sw < W;
      const int ch = min(max(sh, 0), H - 1), cw = min(max(sw, 0), W - 1);
      const unsigned char raw =
          data[(((long)(ok ? i : 0) * H + ch) * W + cw) * C + c];
      const float v = in ? (float)raw : 0.f;
      // selects, not runtime-indexed arrays (those go to scratch)
      const float s = c == 0 ? sc[0] : c == 1 ? sc[1] : c == 2 ? sc[2] : sc[3];
      const float t = c == 0 ? sf[0] : c == 1 ? sf[1] : c == 2 ? sf[2] : sf[3];
      // not contracted (pragma above): the CPU path's mul-then-add
      const float p = v * s;
      o[u] = f32_to_s16<T16>(p + t);
      if (++c == C) {
        c = 0;
        if (++w == W) {
          w = 0;
          if (++h == H) {
            h = 0;
            b = min(b + 1, (long)B - 1);
            i = indices[b];
            ok = (unsigned)i < (unsigned)N;
            d = aug_draw((unsigned)i, key, span, pad, flip);
          }
        }
      }
    }
    if (cnt == 8) {
      *reinterpret_cast<short8*>(x + e0) = o;
    } else {
      short* xs = reinterpret_cast<short*>(x + e0);
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (u < cnt) xs[u] = o[u];
    }
  }
}

// ---------------------------------------------------------------------------
// CutMix / Mixup: the pair batch builder
// ---------------------------------------------------------------------------
// Output position b mixes A[b] with A[B-1-b] (A = what the kernel above
// builds before it normalizes; each sample keeps its own crop and flip).
// The mode, lam and the cutmix box continue the hash chain of b's own
// dataset index (h, h2 above -> h3, h4), so they too are the same at any
// batch size or rank. mi355x.data.mix_params is the twin in numpy.

enum { kMixNone = 0, kMixCut = 1, kMixUp = 2 };

// exact floor(sqrt(n)) for 0 <= n < 2^62: a double guess is off by at most
// one (its relative error is 2^-53 and the root is below 2^31)
DEV_INLINE long isqrt_l(long n) {
  long s = (long)sqrt((double)n);
  if (s * s > n) --s;
  if ((s + 1) * (s + 1) <= n) ++s;
  return s;
}

struct MixDraw {
  int mode;
  float lam;           // weight of the own sample (label weight too)
  int y0, y1, x0, x1;  // cutmix box, clipped to the image; empty otherwise
};

DEV_INLINE MixDraw mix_draw(unsigned i, unsigned key, int H, int W, int tc,
                            int tm, float inv_hw) {
  const unsigned h = mix32(i ^ key);
  const unsigned h2 = mix32(h + 0x9E3779B9u);
  const unsigned h3 = mix32(h2 + 0x9E3779B9u);
  const unsigned h4 = mix32(h3 + 0x9E3779B9u);
  const int r = (int)(h3 & 0xffffu);
  const long u = (long)(h3 >> 16);
  MixDraw m;
  m.mode = r < tc ? kMixCut : r < tc + tm ? kMixUp : kMixNone;
  m.lam = 1.f;
  m.y0 = m.y1 = m.x0 = m.x1 = 0;
  if (m.mode == kMixUp) {
    m.lam = (float)u * (1.f / 65536.f);  // exact: 16 bits times 2^-16
  } else if (m.mode == kMixCut) {
    const long ch = isqrt_l(((long)H * H * (65536 - u)) >> 16);
    const long cw = isqrt_l(((long)W * W * (65536 - u)) >> 16);
    const long cy = ((long)(h4 & 0xffffu) * H) >> 16;
    const long cx = ((long)(h4 >> 16) * W) >> 16;
    m.y0 = (int)max(cy - ch / 2, 0l);
    m.y1 = (int)min(cy - ch / 2 + ch, (long)H);
    m.x0 = (int)max(cx - cw / 2, 0l);
    m.x1 = (int)min(cx - cw / 2 + cw, (long)W);
    const long keep =
        (long)H * W - (long)(m.y1 - m.y0) * (long)(m.x1 - m.x0);
    m.lam = (float)keep * inv_hw;  // one fp32 multiply, as the twin does
  }
  return m;
}

// everything a lane needs to know about output position b
struct MixCtx {
  int i, j;       // own and partner dataset index, clamped to 0 if bad
  bool oki, okj;  // the unclamped index was inside [0,N)
  Draw di, dj;
  MixDraw m;
};

DEV_INLINE MixCtx mix_ctx(long b, const int* __restrict__ indices, int N,
                          int B, int H, int W, unsigned key, unsigned span,
                          int pad, bool flip, int tc, int tm, float inv_hw) {
  MixCtx x;
  const int i = indices[b], j = indices[B - 1 - b];
  x.oki = (unsigned)i < (unsigned)N;
  x.okj = (unsigned)j < (unsigned)N;
  x.di = aug_draw((unsigned)i, key, span, pad, flip);
  x.dj = aug_draw((unsigned)j, key, span, pad, flip);
  x.m = mix_draw((unsigned)i, key, H, W, tc, tm, inv_hw);
  // an index outside the dataset is never used as an address
  x.i = x.oki ? i : 0;
  x.j = x.okj ? j : 0;
  return x;
}

// clamped byte offset of pixel (h,w) inside a sample under draw d (below
// H*W*C, so an int), and whether the pixel lies inside the image (outside:
// padding, raw 0)
DEV_INLINE int src_rel(const Draw& d, int h, int w, int H, int W, int C,
                       bool& in) {
  const int sh = h + d.oy;
  const int sw = (d.f ? W - 1 - w : w) + d.ox;
  in = sh >= 0 && sh < H && sw >= 0 && sw < W;
  const int ch = min(max(sh, 0), H - 1), cw = min(max(sw, 0), W - 1);
  return (ch * W + cw) * C;
}

template <typename T16>
__global__ __launch_bounds__(256) void gather_mix_kernel(
    const unsigned char* __restrict__ data, const long* __restrict__ targets,
    const int* __restrict__ indices, const float* __restrict__ scale,
    const float* __restrict__ shift, T16* __restrict__ x,
    long* __restrict__ ya, long* __restrict__ yb, float* __restrict__ lam,
    int N, int B, int H, int W, int C, int pad, bool flip, unsigned key,
    int tc, int tm, float inv_hw) {
  const int HWC = H * W * C;
  const long total = (long)B * HWC;
  const unsigned span = 2u * (unsigned)pad + 1u;
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long nthr = (long)gridDim.x * blockDim.x;

  for (long b = tid; b < B; b += nthr) {
    const int i = indices[b], j = indices[B - 1 - b];
    const MixDraw m = mix_draw((unsigned)i, key, H, W, tc, tm, inv_hw);
    // an index outside the dataset reads nothing: label -1 in its slot
    const long la = (unsigned)i < (unsigned)N ? targets[i] : -1;
    const long lb = (unsigned)j < (unsigned)N ? targets[j] : -1;
    ya[b] = la;
    yb[b] = m.mode == kMixNone ? la : lb;
    lam[b] = m.lam;
  }

  float sc[4], sf[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    sc[c] = c < C ? scale[c] : 0.f;
    sf[c] = c < C ? shift[c] : 0.f;
  }

  for (long e0 = tid * 8; e0 < total; e0 += nthr * 8) {
    // (b,h,w,c) of the first element; the others follow by carry
    long b = e0 / HWC;
    const int r0 = (int)(e0 - b * HWC);
    int r = r0;
    int h = r / (W * C);
    r -= h * (W * C);
    int w = r / C;
    int c = r - w * C;
    MixCtx s =
        mix_ctx(b, indices, N, B, H, W, key, span, pad, flip, tc, tm, inv_hw);

    if (r0 + 8 > HWC) {
      // The lane's elements run past the end of its sample (into the next
      // one, or off the end of the batch): possible only where a sample is
      // no multiple of 8 elements, and then for one lane per sample. One
      // element at a time, redrawing at the boundary; not unrolled, so the
      // draws are not replicated and the registers of the path below set
      // the occupancy.
      const int cnt = (int)(total - e0 < 8 ? total - e0 : 8);
      short* xs = reinterpret_cast<short*>(x + e0);
#pragma unroll 1
      for (int u = 0; u < cnt; ++u) {
        const bool box = s.m.mode == kMixCut && h >= s.m.y0 && h < s.m.y1 &&
                         w >= s.m.x0 && w < s.m.x1;
        bool in, inj;
        const long off = (long)(box ? s.j : s.i) * HWC +
                         src_rel(box ? s.dj : s.di, h, w, H, W, C, in);
        in = in && (box ? s.okj : s.oki);
        const long offj = (long)s.j * HWC + src_rel(s.dj, h, w, H, W, C, inj);
        inj = inj && s.okj;
        // clamped in-range addresses, then selects
        const float a = in ? (float)data[off + c] : 0.f;
        const float p = inj ? (float)data[offj + c] : 0.f;
        const float wl = s.m.mode == kMixUp ? s.m.lam : 1.f;
        const float v = a * wl + p * (1.f - wl);
        const float sv = c == 0 ? sc[0] : c == 1 ? sc[1] : c == 2 ? sc[2] : sc[3];
        const float tv = c == 0 ? sf[0] : c == 1 ? sf[1] : c == 2 ? sf[2] : sf[3];
        const float q = v * sv;
        xs[u] = f32_to_s16<T16>(q + tv);
        if (++c == C) {
          c = 0;
          if (++w == W) {
            w = 0;
            if (++h == H) {
              h = 0;
              // u + 1 < cnt here, so b + 1 < B
              b = min(b + 1, (long)B - 1);
              s = mix_ctx(b, indices, N, B, H, W, key, span, pad, flip, tc,
                          tm, inv_hw);
            }
          }
        }
      }
      continue;
    }

    // All 8 elements lie in sample b: the mode, the weight and the draws
    // are the lane's, only (h,w,c) walk. First gather of every element: a
    // none or cutmix pixel has one source (chosen before the load), a mixup
    // pixel starts with its own sample. The arrays are compile-time indexed
    // after the unroll, so they stay in registers.
    const bool up = s.m.mode == kMixUp;
    const float wl = up ? s.m.lam : 1.f;  // the own sample's weight
    const unsigned char* own = data + (long)s.i * HWC;
    const unsigned char* par = data + (long)s.j * HWC;
    float a[8];
    int rel2[8];
    bool in2[8];
    const int c0 = c;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const bool box = s.m.mode == kMixCut && h >= s.m.y0 && h < s.m.y1 &&
                       w >= s.m.x0 && w < s.m.x1;
      bool in;
      const int rel = src_rel(box ? s.dj : s.di, h, w, H, W, C, in);
      in = in && (box ? s.okj : s.oki);
      // always a clamped in-range address, then a select: the 8 byte
      // gathers of a lane are in flight together
      const unsigned char raw = (box ? par : own)[rel + c];
      a[u] = in ? (float)raw : 0.f;
      bool inj;
      rel2[u] = src_rel(s.dj, h, w, H, W, C, inj) + c;
      in2[u] = inj && s.okj;
      if (++c == C) {
        c = 0;
        if (++w == W) {
          w = 0;
          ++h;  // stays below H: the 8 elements end inside the sample
        }
      }
    }
    // second gather, only for a mixup sample
    float p[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) p[u] = 0.f;
    if (up) {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const unsigned char raw = par[rel2[u]];
        p[u] = in2[u] ? (float)raw : 0.f;
      }
    }
    short8 o;
    int cc = c0;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      // exact in fp32: each product is an 8-bit value times a 17-bit
      // weight over 2^16, and their sum stays below 2^24 (with wl = 1 it
      // is a[u] itself)
      const float v = a[u] * wl + p[u] * (1.f - wl);
      const float sv =
          cc == 0 ? sc[0] : cc == 1 ? sc[1] : cc == 2 ? sc[2] : sc[3];
      const float tv =
          cc == 0 ? sf[0] : cc == 1 ? sf[1] : cc == 2 ? sf[2] : sf[3];
      // not contracted (pragma above): the CPU path's mul-then-add
      const float q = v * sv;
      o[u] = f32_to_s16<T16>(q + tv);
      if (++cc == C) cc = 0;
    }
    *reinterpret_cast<short8*>(x + e0) = o;
  }
}

// same cap as elementwise.hip's ew_grid
inline int aug_grid(long n, int per_thread, int block = 256) {
  long blocks = cdiv_l(n, (long)block * per_thread);
  return (int)std::max<long>(1, std::min<long>(blocks, 2048));
}

}  // namespace

// tc, tm: the mode thresholds round(p*65536) of cutmix and mixup; inv_hw:
// float32(1/(H*W)). Both come from the Python side, which is also where the
// CPU twin takes them from, so the two cannot round differently.
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> gather_augment_mix(
    at::Tensor data_u8, at::Tensor targets, at::Tensor indices,
    at::Tensor scale, at::Tensor shift, int64_t pad, bool flip, int64_t tc,
    int64_t tm, double inv_hw, int64_t seed, int64_t epoch, at::Tensor like) {
  CHECK_GPU(data_u8);
  CHECK_GPU(targets);
  CHECK_GPU(indices);
  CHECK_GPU(scale);
  CHECK_GPU(shift);
  CHECK_CONTIG(data_u8);
  CHECK_CONTIG(targets);
  CHECK_CONTIG(indices);
  CHECK_CONTIG(scale);
  CHECK_CONTIG(shift);
  CHECK_16BIT(like);
  TORCH_CHECK(data_u8.scalar_type() == at::kByte && data_u8.dim() == 4,
              "data_u8 must be (N,H,W,C) uint8");
  TORCH_CHECK(targets.scalar_type() == at::kLong && targets.dim() == 1 &&
                  targets.size(0) == data_u8.size(0),
              "targets must be (N,) int64");
  TORCH_CHECK(indices.scalar_type() == at::kInt && indices.dim() == 1 &&
                  indices.size(0) >= 1,
              "indices must be (B,) int32 with B >= 1");
  const long N = data_u8.size(0), H = data_u8.size(1), W = data_u8.size(2),
             C = data_u8.size(3), B = indices.size(0);
  TORCH_CHECK(C >= 1 && C <= 4,
              "gather_augment_mix supports 1..4 channels, got ", C);
  TORCH_CHECK(scale.scalar_type() == at::kFloat && scale.numel() == C &&
                  shift.scalar_type() == at::kFloat && shift.numel() == C,
              "scale and shift must be (C,) float32");
  TORCH_CHECK(N >= 1 && N <= INT_MAX && B <= INT_MAX && H >= 1 && W >= 1 &&
                  H * W * C <= INT_MAX,
              "gather_augment_mix: dataset or sample too large");
  // the box size is isqrt((H*H*(65536-u)) >> 16) in int64
  TORCH_CHECK(H <= (1l << 23) && W <= (1l << 23),
              "gather_augment_mix: H and W must be at most 2^23");
  TORCH_CHECK(pad >= 0 && pad <= 32767, "pad must be in [0, 32767], got ", pad);
  TORCH_CHECK(tc >= 0 && tm >= 0 && tc + tm <= 65536,
              "gather_augment_mix: thresholds must be >= 0 and sum to at most "
              "65536, got ", tc, " and ", tm);
  const unsigned key =
      mix32((unsigned)(uint64_t)seed * 0x9E3779B9u + (unsigned)(uint64_t)epoch);

  auto x = at::empty({B, H, W, C}, like.options().device(data_u8.device()));
  auto ya = at::empty({B}, targets.options());
  auto yb = at::empty({B}, targets.options());
  auto lam = at::empty({B}, targets.options().dtype(at::kFloat));
  const long total = B * H * W * C;
  DISPATCH_16(like, T16, {
    hipLaunchKernelGGL(gather_mix_kernel<T16>, dim3(aug_grid(total, 8)),
                       dim3(256), 0, cur_stream(),
                       data_u8.data_ptr<unsigned char>(),
                       targets.data_ptr<long>(), indices.data_ptr<int>(),
                       scale.data_ptr<float>(), shift.data_ptr<float>(),
                       (T16*)x.data_ptr(), ya.data_ptr<long>(),
                       yb.data_ptr<long>(), lam.data_ptr<float>(), (int)N,
                       (int)B, (int)H, (int)W, (int)C, (int)pad, flip, key,
                       (int)tc, (int)tm, (float)inv_hw);
  });
  return {x, ya, yb, lam};
}

std::tuple<at::Tensor, at::Tensor> gather_augment(
    at::Tensor data_u8, at::Tensor targets, at::Tensor indices,
    at::Tensor scale, at::Tensor shift, int64_t pad, bool flip, int64_t seed,
    int64_t epoch, at::Tensor like) {
  CHECK_GPU(data_u8);
  CHECK_GPU(targets);
  CHECK_GPU(indices);
  CHECK_GPU(scale);
  CHECK_GPU(shift);
  CHECK_CONTIG(data_u8);
  CHECK_CONTIG(targets);
  CHECK_CONTIG(indices);
  CHECK_CONTIG(scale);
  CHECK_CONTIG(shift);
  CHECK_16BIT(like);
  TORCH_CHECK(data_u8.scalar_type() == at::kByte && data_u8.dim() == 4,
              "data_u8 must be (N,H,W,C) uint8");
  TORCH_CHECK(targets.scalar_type() == at::kLong && targets.dim() == 1 &&
                  targets.size(0) == data_u8.size(0),
              "targets must be (N,) int64");
  TORCH_CHECK(indices.scalar_type() == at::kInt && indices.dim() == 1 &&
                  indices.size(0) >= 1,
              "indices must be (B,) int32 with B >= 1");
  const long N = data_u8.size(0), H = data_u8.size(1), W = data_u8.size(2),
             C = data_u8.size(3), B = indices.size(0);
  TORCH_CHECK(C >= 1 && C <= 4, "gather_augment supports 1..4 channels, got ",
              C);
  TORCH_CHECK(scale.scalar_type() == at::kFloat && scale.numel() == C &&
                  shift.scalar_type() == at::kFloat && shift.numel() == C,
              "scale and shift must be (C,) float32");
  TORCH_CHECK(N >= 1 && N <= INT_MAX && B <= INT_MAX && H >= 1 && W >= 1 &&
                  H * W * C <= INT_MAX,
              "gather_augment: dataset or sample too large");
  // dy/dx are 16.16 fixed-point products in uint32: (2*pad+1)*0xffff < 2^32
  TORCH_CHECK(pad >= 0 && pad <= 32767, "pad must be in [0, 32767], got ", pad);
  const unsigned key =
      mix32((unsigned)(uint64_t)seed * 0x9E3779B9u + (unsigned)(uint64_t)epoch);

  auto x = at::empty({B, H, W, C}, like.options().device(data_u8.device()));
  auto y = at::empty({B}, targets.options());
  const long total = B * H * W * C;
  DISPATCH_16(like, T16, {
    hipLaunchKernelGGL(gather_augment_kernel<T16>, dim3(aug_grid(total, 8)),
                       dim3(256), 0, cur_stream(),
                       data_u8.data_ptr<unsigned char>(),
                       targets.data_ptr<long>(), indices.data_ptr<int>(),
                       scale.data_ptr<float>(), shift.data_ptr<float>(),
                       (T16*)x.data_ptr(), y.data_ptr<long>(), (int)N, (int)B,
                       (int)H, (int)W, (int)C, (int)pad, flip, key);
  });
  return {x, y};
}
