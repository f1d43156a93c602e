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

// same cap as elementwise.hip's ew_grid
inline int aug_grid(long n, int per_thread, int block = 256) {
  long blocks = cdiv_l(n, (long)block * per_thread);
  return (int)std::max<long>(1, std::min<long>(blocks, 2048));
}

}  // namespace

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
