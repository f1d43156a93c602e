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

// ---------------------------------------------------------------------------
// Random resized crop + bilinear resize: the resampling batch builder
// ---------------------------------------------------------------------------
// One source sample now feeds an output many times its size (3 KB -> 300 KB
// for 32x32x3 -> 224x224x3), so the work is split the other way round from
// the kernels above: a 256-thread block owns one sample and a band of R
// output rows (grid = bands x B), stages the source rows the band needs in
// LDS once, and everything a lane would otherwise recompute per element is
// done once per block (draws, crop box, column map) or once per output row
// (row map). The arithmetic is integer up to the normalize, so
// mi355x.data.rrc_params and the CPU op are bit-equal twins.
//
//   1. thread 0: draws -> crop box (y0,x0,ch,cw,flip), first source row and
//      row count of the band, into LDS
//   2. column map (one packed word per output column: source element
//      offset, whether a right neighbour exists, fx; mirrored for a flipped
//      sample), row map (one word per output row of the band), and the
//      source rows as 16-byte global loads of the aligned byte range that
//      holds them
//   3. per output row, one wave blends its two source rows into a row of
//      cw*C uint16 (raw*wy <= 255*256)
//   4. a lane builds 8 consecutive output elements from two LDS values each
//      and stores 16 bytes. The band is walked as one flat element range in
//      16-byte-aligned chunks, so a row length that is no multiple of 8 only
//      costs element stores in the band's first and last chunk.
//
// wx*(r00*wy0 + r10*wy1) + wx1*(r01*wy0 + r11*wy1) is the four-tap sum of
// the semantics, integer for integer. No division and no hash in 3 or 4.
//
// LDS (dynamic, see ResizeLds): staged rows + R blended rows + maps. The
// host halves R from 16 until that is at most 20 KB, which keeps 8 blocks
// (the 32-wave limit) on a CU's 160 KB; a wide source (W*C up to 8192
// bytes) ends at R = 1 and up to 56 KB, 2 blocks per CU. 32x32x3 -> 224
// takes 4.5 KB at R = 16; 48 VGPRs at most, no scratch, 8 waves per SIMD.
// Times, the band heights tried and the write floor:
// profiles/r22_resized_loader.md.

struct Box {
  int y0, x0, ch, cw;
  bool f;
};

// the crop box and flip of dataset sample i; the whole image when !rrc
DEV_INLINE Box rrc_draw(unsigned i, unsigned key, int H, int W, bool rrc,
                        int lo_q, int hi_q, const int* __restrict__ ratio_q16,
                        bool flip) {
  Box b;
  b.y0 = b.x0 = 0;
  b.ch = H;
  b.cw = W;
  b.f = false;
  if (!rrc) return b;
  const unsigned h = mix32(i ^ key);
  const unsigned h2 = mix32(h + 0x9E3779B9u);
  const unsigned h3 = mix32(h2 + 0x9E3779B9u);
  const unsigned h4 = mix32(h3 + 0x9E3779B9u);
  const unsigned h5 = mix32(h4 + 0x9E3779B9u);
  const unsigned h6 = mix32(h5 + 0x9E3779B9u);
  b.f = flip && (h2 & 1u);
  // area in Q16 of the image, then one log-uniform aspect ratio from the
  // host's table: one draw, clamped (no retries)
  const long aq =
      lo_q + (long)(((h5 & 0xffffu) * (unsigned)(hi_q - lo_q + 1)) >> 16);
  const long A = max(1l, ((long)H * W * aq) >> 16);
  const long rq = ratio_q16[h5 >> 24];
  b.cw = (int)min(max(isqrt_l((A * rq) >> 16), 1l), (long)W);
  b.ch = (int)min(max(isqrt_l((A << 16) / rq), 1l), (long)H);
  b.y0 = (int)(((h6 & 0xffffu) * (unsigned)(H - b.ch + 1)) >> 16);
  b.x0 = (int)(((h6 >> 16) * (unsigned)(W - b.cw + 1)) >> 16);
  return b;
}

// Q16 source coordinate of output pixel o (pixel centres, edges replicated)
DEV_INLINE int src_q16(int o, int n_src, int n_out) {
  const long s = ((long)(2 * o + 1) * n_src * 32768) / n_out - 32768;
  return (int)min(max(s, 0l), (long)(n_src - 1) << 16);
}

// Rows of source a band of R output rows can touch, for any crop height up
// to H: the band's first and last source row differ by at most
// ceil((R-1)*ch/OH), and one more row below the last is its second tap.
__host__ __device__ inline int resize_cap_rows(int R, int H, int OH) {
  const long c = ((long)(R - 1) * H) / OH + 3;
  return (int)(c < H ? c : H);
}

// byte offsets of the kernel's LDS sections; the host sizes the launch
// from the same struct
struct ResizeLds {
  int stage, blend, colmap, rowmap, prm, total, bstride;
  __host__ __device__ ResizeLds(int R, int cap_rows, int WC, int OW) {
    stage = 0;
    // up to 15 bytes in front of the rows (16-byte aligned loads), whole
    // 16-byte chunks
    blend = (15 + cap_rows * WC + 15) & ~15;
    bstride = (WC + 1) & ~1;  // uint16 elements per blended row
    colmap = blend + R * bstride * 2;
    rowmap = colmap + OW * 4;
    prm = rowmap + R * 4;
    total = prm + 32;
  }
};

constexpr int kResizeLdsTarget = 20 * 1024;  // 8 blocks on a 160 KB CU
constexpr int kResizeLdsMax = 64 * 1024;

// one output element from its blended row
template <typename T16, int C>
DEV_INLINE short resize_pix(const unsigned short* __restrict__ bl,
                            unsigned cm, int c, float s, float t) {
  const int e0 = (int)(cm & 0x3fffu) + c;
  const int e1 = e0 + ((cm >> 14) & 1u ? C : 0);
  const int fx = (int)(cm >> 16);
  const int val = (int)bl[e0] * (256 - fx) + (int)bl[e1] * fx;
  // at most 255 * 2^16: exact in fp32, and so is the 2^-16
  const float v = (float)val * (1.f / 65536.f);
  // not contracted (pragma above): the CPU path's mul-then-add
  const float p = v * s;
  return f32_to_s16<T16>(p + t);
}

template <typename T16, int C>
__global__ __launch_bounds__(256) void gather_resize_kernel(
    const unsigned char* __restrict__ data, const long* __restrict__ targets,
    const int* __restrict__ indices, const float* __restrict__ scale,
    const float* __restrict__ shift, const int* __restrict__ ratio_q16,
    T16* __restrict__ x, long* __restrict__ y, int N, int H, int W, int OH,
    int OW, int R, int cap_rows, bool rrc, int lo_q, int hi_q, bool flip,
    unsigned key) {
  extern __shared__ __align__(16) unsigned char lds[];
  const int WC = W * C, OWC = OW * C;
  const ResizeLds L(R, cap_rows, WC, OW);
  unsigned char* stage = lds + L.stage;
  unsigned short* blend = reinterpret_cast<unsigned short*>(lds + L.blend);
  unsigned* colmap = reinterpret_cast<unsigned*>(lds + L.colmap);
  unsigned* rowmap = reinterpret_cast<unsigned*>(lds + L.rowmap);
  int* prm = reinterpret_cast<int*>(lds + L.prm);

  const int tid = threadIdx.x, b = blockIdx.y, oy0 = blockIdx.x * R;
  const int rows = min(R, OH - oy0);
  const int i = indices[b];
  // an index outside the dataset reads nothing: label -1, raw 0 everywhere
  const bool ok = (unsigned)i < (unsigned)N;

  if (tid == 0) {
    const Box bx =
        rrc_draw((unsigned)i, key, H, W, rrc, lo_q, hi_q, ratio_q16, flip);
    const int iy_first = src_q16(oy0, bx.ch, OH) >> 16;
    const int iy_last = src_q16(oy0 + rows - 1, bx.ch, OH) >> 16;
    prm[0] = bx.y0;
    prm[1] = bx.x0;
    prm[2] = bx.ch;
    prm[3] = bx.cw;
    prm[4] = bx.f;
    prm[5] = iy_first;
    // never more than the launch reserved (resize_cap_rows is the bound)
    prm[6] = min(min(iy_last + 1, bx.ch - 1) - iy_first + 1, cap_rows);
    if (blockIdx.x == 0) y[b] = ok ? targets[i] : -1;
  }
  __syncthreads();
  const int y0 = prm[0], x0 = prm[1], ch = prm[2], cw = prm[3];
  const bool f = prm[4] != 0;
  const int iy_first = prm[5], nsrc = prm[6];

  for (int ox = tid; ox < OW; ox += 256) {
    const int sx = src_q16(f ? OW - 1 - ox : ox, cw, OW);
    const int ix = sx >> 16, fx = (sx >> 8) & 255;
    colmap[ox] = (unsigned)(ix * C) | (ix + 1 < cw ? 1u << 14 : 0u) |
                 (unsigned)fx << 16;
  }
  if (tid < rows) {
    const int sy = src_q16(oy0 + tid, ch, OH);
    const int iy = sy >> 16, fy = (sy >> 8) & 255;
    const int r0 = min(iy - iy_first, nsrc - 1);
    const int r1 = min(min(iy + 1, ch - 1) - iy_first, nsrc - 1);
    rowmap[tid] = (unsigned)r0 | (unsigned)(r1 - r0) << 13 | (unsigned)fy << 16;
  }
  // Source rows y0+iy_first .. +nsrc-1, whole rows: one contiguous byte
  // range of the sample. It is loaded as the 16-byte-aligned chunks that
  // cover it; a chunk that sticks out of the dataset (possible only at its
  // two ends) is read byte by byte, inside bytes only.
  const long s_off = ((long)(ok ? i : 0) * H + y0 + iy_first) * WC;
  const int head = (int)(reinterpret_cast<uintptr_t>(data + s_off) & 15);
  if (ok) {
    const unsigned char* abase = data + s_off - head;
    const unsigned char* dend = data + (long)N * H * WC;
    const int nchunk = (head + nsrc * WC + 15) >> 4;
    for (int k = tid; k < nchunk; k += 256) {
      const unsigned char* p = abase + 16 * k;
      if (p >= data && p + 16 <= dend) {
        *reinterpret_cast<int4v*>(stage + 16 * k) =
            *reinterpret_cast<const int4v*>(p);
      } else {
#pragma unroll 1
        for (int u = 0; u < 16; ++u)
          stage[16 * k + u] = (p + u >= data && p + u < dend) ? p[u] : 0;
      }
    }
  }
  __syncthreads();

  // one wave per output row: the two source rows, weighted, as uint16
  const int cwC = cw * C;
  for (int j = tid >> 6; j < rows; j += 4) {
    const unsigned rm = rowmap[j];
    const int fy = (int)(rm >> 16);
    const unsigned char* s0 = stage + head + (int)(rm & 0x1fffu) * WC + x0 * C;
    const unsigned char* s1 = s0 + ((rm >> 13) & 1u ? WC : 0);
    unsigned short* bl = blend + j * L.bstride;
    for (int e = tid & 63; e < cwC; e += 64)
      bl[e] = ok ? (unsigned short)(s0[e] * (256 - fy) + s1[e] * fy) : 0;
  }
  __syncthreads();

  float sc[4], sf[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    sc[c] = c < C ? scale[c] : 0.f;
    sf[c] = c < C ? shift[c] : 0.f;
  }

  // The band's elements are one flat range of x. Chunk q is the 8 elements
  // at the 16-byte-aligned address xa + 8q; rel is its first element
  // relative to the band (negative in chunk 0 if the band starts inside a
  // chunk), (j, m) the row and the position in the row of that element,
  // stepped by 2048 elements per round without a division.
  const long band0 = ((long)b * OH + oy0) * OWC;
  const int ohead = (int)(band0 & 7);
  short* xa = reinterpret_cast<short*>(x) + (band0 - ohead);
  const int total = rows * OWC;
  const int nq = (ohead + total + 7) >> 3;
  const int step_j = 2048 / OWC, step_m = 2048 - step_j * OWC;
  int rel = 8 * tid - ohead;
  int j = rel >= 0 ? rel / OWC : -((-rel + OWC - 1) / OWC);
  int m = rel - j * OWC;
  for (int q = tid; q < nq; q += 256) {
    if (rel >= 0 && rel + 8 <= total) {
      const unsigned short* bl = blend + j * L.bstride;
      int ox = m / C, c = m - ox * C, mm = m;
      short8 o;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        // selects, not runtime-indexed arrays (those go to scratch)
        const float s = c == 0 ? sc[0] : c == 1 ? sc[1] : c == 2 ? sc[2] : sc[3];
        const float t = c == 0 ? sf[0] : c == 1 ? sf[1] : c == 2 ? sf[2] : sf[3];
        o[u] = resize_pix<T16, C>(bl, colmap[ox], c, s, t);
        if (++c == C) {
          c = 0;
          ++ox;
        }
        if (++mm == OWC) {  // next row of the band
          mm = 0;
          ox = 0;
          c = 0;
          bl += L.bstride;
        }
      }
      *reinterpret_cast<short8*>(xa + 8 * q) = o;
    } else {
      // the band's first or last chunk: only the elements inside the band
#pragma unroll 1
      for (int u = 0; u < 8; ++u) {
        const int r = rel + u;
        if (r < 0 || r >= total) continue;
        const int jj = r / OWC, m2 = r - jj * OWC;
        const int ox = m2 / C, c = m2 - ox * C;
        const float s = c == 0 ? sc[0] : c == 1 ? sc[1] : c == 2 ? sc[2] : sc[3];
        const float t = c == 0 ? sf[0] : c == 1 ? sf[1] : c == 2 ? sf[2] : sf[3];
        xa[8 * q + u] =
            resize_pix<T16, C>(blend + jj * L.bstride, colmap[ox], c, s, t);
      }
    }
    rel += 2048;
    j += step_j;
    m += step_m;
    if (m >= OWC) {
      m -= OWC;
      ++j;
    }
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

// Random resized crop + bilinear resize to (OH, OW). rrc: draw a crop box
// per sample (lo_q, hi_q: the area bounds round(scale*65536); ratio_q16:
// the 256-entry log-uniform aspect table, int32 on the device; flip as in
// gather_augment); without it the whole image is resized and nothing is
// drawn. band_rows: output rows per block, 0 for the default of 16; either
// is halved until the block's LDS is within kResizeLdsTarget.
//
// Domain of the LDS staging: C in 1..4, H and W at most 4096, output sides
// in [1, 4096], W*C at most 8192 bytes (then even a one-row band, which
// needs 3 staged rows, 1 blended row and the maps, fits 64 KB), B at most
// 65535 (the grid's second dimension).
std::tuple<at::Tensor, at::Tensor> gather_resize(
    at::Tensor data_u8, at::Tensor targets, at::Tensor indices,
    at::Tensor scale, at::Tensor shift, int64_t OH, int64_t OW, bool rrc,
    int64_t lo_q, int64_t hi_q, c10::optional<at::Tensor> ratio_q16, bool flip,
    int64_t seed, int64_t epoch, int64_t band_rows, at::Tensor like) {
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
  TORCH_CHECK(C >= 1 && C <= 4, "gather_resize supports 1..4 channels, got ",
              C);
  TORCH_CHECK(scale.scalar_type() == at::kFloat && scale.numel() == C &&
                  shift.scalar_type() == at::kFloat && shift.numel() == C,
              "scale and shift must be (C,) float32");
  TORCH_CHECK(H >= 1 && H <= 4096 && W >= 1 && W <= 4096,
              "gather_resize: H and W must be in [1, 4096], got ", H, " x ",
              W);
  TORCH_CHECK(OH >= 1 && OH <= 4096 && OW >= 1 && OW <= 4096,
              "gather_resize: output sides must be in [1, 4096], got ", OH,
              " x ", OW);
  TORCH_CHECK(W * C <= 8192, "gather_resize: a source row of W*C = ", W * C,
              " bytes does not fit the LDS staging (at most 8192)");
  TORCH_CHECK(N >= 1 && N <= INT_MAX && B <= 65535,
              "gather_resize: N must be in [1, 2^31) and B at most 65535, got ",
              N, " and ", B);
  TORCH_CHECK(band_rows >= 0 && band_rows <= 64,
              "gather_resize: band_rows must be in [0, 64], got ", band_rows);
  const int* ratio = nullptr;
  if (rrc) {
    TORCH_CHECK(lo_q >= 1 && lo_q <= hi_q && hi_q <= 65536,
                "gather_resize: need 1 <= lo_q <= hi_q <= 65536, got ", lo_q,
                " and ", hi_q);
    TORCH_CHECK(ratio_q16.has_value(), "gather_resize: rrc needs ratio_q16");
    const at::Tensor& r = *ratio_q16;
    CHECK_GPU(r);
    CHECK_CONTIG(r);
    TORCH_CHECK(r.scalar_type() == at::kInt && r.numel() == 256,
                "ratio_q16 must be 256 int32 values");
    ratio = r.data_ptr<int>();
  }
  const unsigned key =
      mix32((unsigned)(uint64_t)seed * 0x9E3779B9u + (unsigned)(uint64_t)epoch);

  int R = (int)std::min<long>(band_rows ? band_rows : 16, OH);
  auto lds_of = [&](int r) {
    return ResizeLds(r, resize_cap_rows(r, (int)H, (int)OH), (int)(W * C),
                     (int)OW).total;
  };
  while (R > 1 && lds_of(R) > kResizeLdsTarget) R = (R + 1) / 2;
  const int lds_bytes = lds_of(R);
  TORCH_CHECK(lds_bytes <= kResizeLdsMax, "gather_resize: ", lds_bytes,
              " bytes of LDS for W*C = ", W * C, " and OW = ", OW);

  auto x = at::empty({B, OH, OW, C}, like.options().device(data_u8.device()));
  auto y = at::empty({B}, targets.options());
  const dim3 grid((unsigned)cdiv_l(OH, R), (unsigned)B);
  DISPATCH_16(like, T16, {
    pick<1, 2, 3, 4>((int)C, [&](auto CC) {
      launch256(gather_resize_kernel<T16, CC>, grid, (size_t)lds_bytes,
                data_u8.data_ptr<unsigned char>(), targets.data_ptr<long>(),
                indices.data_ptr<int>(), scale.data_ptr<float>(),
                shift.data_ptr<float>(), ratio, (T16*)x.data_ptr(),
                y.data_ptr<long>(), (int)N, (int)H, (int)W, (int)OH, (int)OW,
                R, resize_cap_rows(R, (int)H, (int)OH), rrc, (int)lo_q,
                (int)hi_q, flip, key);
    });
  });
  return {x, y};
}
