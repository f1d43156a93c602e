// Shared epilogue store of the MFMA conv kernels (conv_mfma.hip,
// stem_mfma.hip): a block's accumulator tile leaves as whole output rows,
// 16 bytes per lane, instead of one 16-bit element per lane.
//
// The 32x32 MFMA accumulator puts the output channel on the lane and the
// output row in the register, so a direct store writes 2 bytes per lane:
// 32 store instructions per wave for a 32 x 64 tile. Here each of the
// block's four waves stages its 32-row x (32*NT)-channel tile, already
// rounded to 16 bit, in a wave-private region of LDS that the main loop no
// longer needs, and reads it back so that NT*4 consecutive lanes cover one
// row's channels in 16-byte pieces: 4 (NT=2) or 8 (NT=4) dwordx4 stores per
// wave. A residual ADDIN tile travels the other way first (16-byte global
// loads into the same region, each lane then picks up its own elements), so
// the add stays in fp32 registers and the value is rounded once.
//
// Channel order: the kernels stage weight row n of their B tile at LDS row
// epi_brow<NT>(n), which makes accumulator tile t of lane li hold channel
// li*NT + t of the block's channel range. A lane's NT values are then
// adjacent in the output row and move as one 4- or 8-byte LDS access. Each
// output element is still the same dot product, accumulated in the same
// order.
#pragma once

#include "common.h"

typedef __attribute__((ext_vector_type(2))) short short2v;

// ROWS: tile rows staged per pass. 32 is the whole tile; a kernel with
// less LDS to spare stages 16 (accumulator registers 0-7, then 8-15).
template <int NT, int ROWS = 32>
struct EpiTile {
  static constexpr int RS = NT * 32 + 8;  // staged row stride (+16 B pad)
  static constexpr int LPR = NT * 4;      // lanes per output row, 16 B each
  static constexpr int RPI = 64 / LPR;    // rows per wave instruction
  static constexpr int NIT = ROWS / RPI;  // 16-byte accesses per lane
  static constexpr int WAVE = ROWS * RS;  // elements of one wave's region
  static constexpr int BYTES = 4 * WAVE * 2;  // LDS bytes a block needs
};

template <int NT>
struct EpiPack {};
template <>
struct EpiPack<2> {
  typedef short2v type;
};
template <>
struct EpiPack<4> {
  typedef short4v type;
};

// Orders a wave's LDS writes before its later LDS reads of what its other
// lanes wrote. A wave's region is private to it and the LDS serves one
// wave's accesses in issue order, so no block barrier is needed: the wait
// retires the writes and the memory clobber keeps the compiler from moving
// LDS accesses across this point.
DEV_INLINE void epi_wave_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// LDS row of the B tile that holds weight row (output channel) n
template <int NT>
DEV_INLINE int epi_brow(int n) {
  return (n % NT) * 32 + n / NT;
}

// accumulator register -> row of the wave's tile (32x32 MFMA C layout)
DEV_INLINE int epi_acc_row(int reg, int kh) {
  return (reg & 3) + 8 * (reg >> 2) + 4 * kh;
}

// row of the wave's tile that this lane moves in 16-byte access `it`
template <int NT>
DEV_INLINE int epi_io_row(int it, int lane) {
  return it * EpiTile<NT>::RPI + lane / EpiTile<NT>::LPR;
}

// global -> LDS: the wave's tile of `g`, 16 bytes per lane. roff[it] is the
// element offset in `g` of the first channel of row epi_io_row(it), or
// negative for a row outside the tensor (staged as zeros, never read).
template <typename T16, int NT, int ROWS = 32>
DEV_INLINE void epi_fetch(short* wl, const T16* __restrict__ g, int lane,
                          const long (&roff)[EpiTile<NT, ROWS>::NIT]) {
  using E = EpiTile<NT, ROWS>;
  const int c = (lane % E::LPR) * 8;
  short8 v[E::NIT];
#pragma unroll
  for (int it = 0; it < E::NIT; ++it)
    v[it] = roff[it] >= 0
                ? *reinterpret_cast<const short8*>(g + roff[it] + c)
                : short8{};
#pragma unroll
  for (int it = 0; it < E::NIT; ++it)
    *reinterpret_cast<short8*>(wl + epi_io_row<NT>(it, lane) * E::RS + c) =
        v[it];
}

// the lane's own NT adjacent channels of tile row `row`
template <int NT>
DEV_INLINE typename EpiPack<NT>::type epi_get(const short* wl, int row,
                                              int li) {
  return *reinterpret_cast<const typename EpiPack<NT>::type*>(
      wl + row * EpiTile<NT>::RS + li * NT);
}

template <int NT>
DEV_INLINE void epi_put(short* wl, int row, int li,
                        typename EpiPack<NT>::type h) {
  *reinterpret_cast<typename EpiPack<NT>::type*>(
      wl + row * EpiTile<NT>::RS + li * NT) = h;
}

// LDS -> global: whole rows, 16 bytes per lane; rows with roff < 0 are
// skipped (the M tail)
template <typename T16, int NT, int ROWS = 32>
DEV_INLINE void epi_flush(const short* wl, T16* __restrict__ g, int lane,
                          const long (&roff)[EpiTile<NT, ROWS>::NIT]) {
  using E = EpiTile<NT, ROWS>;
  const int c = (lane % E::LPR) * 8;
#pragma unroll
  for (int it = 0; it < E::NIT; ++it) {
    const short8 v = *reinterpret_cast<const short8*>(
        wl + epi_io_row<NT>(it, lane) * E::RS + c);
    if (roff[it] >= 0) *reinterpret_cast<short8*>(g + roff[it] + c) = v;
  }
}
