// Cross-file declarations of the conv host code (conv.hip dispatches;
// conv_mfma.hip and stem_mfma.hip define the launchers).
#pragma once

#include "common.h"

// ---- conv_mfma.hip: MFMA implicit-GEMM path for C%64==0 && K%64==0 ------
bool conv_mfma_supported(long CI, long KO);
at::Tensor conv_zero_page(const at::Tensor& like);
void wgrad_reduce_launch(at::Tensor part, at::Tensor dw, long E, long nz);
void stats_slab_reduce(at::Tensor slab, at::Tensor stats, int gx, int bnt2,
                       int C);
void conv_fwd_mfma_launch(at::Tensor x, at::Tensor w, at::Tensor bias,
                          at::Tensor y, long stride, long pad, long act,
                          at::Tensor stats, at::Tensor asc, at::Tensor ash);
void conv_fwd_mfma_genc_launch(at::Tensor x, at::Tensor wpad, at::Tensor bias,
                               at::Tensor y, long R, long S, long stride,
                               long pad, long act);
void conv_dgrad_mfma_launch(at::Tensor dy, at::Tensor wflip, at::Tensor dx,
                            long R, long S, long stride, long pad,
                            at::Tensor addin);
void conv_wgrad_mfma_launch(at::Tensor x, at::Tensor dy, at::Tensor dw,
                            long R, long S, long stride, long pad,
                            at::Tensor asc, at::Tensor ash);

// ---- stem_mfma.hip: MFMA GEMM stems (7x7/s2 and 3x3/s1, C=3) ------------
bool conv_fwd_stem_gemm_launch(at::Tensor x, at::Tensor w, at::Tensor bias,
                               at::Tensor y, long pad, long act,
                               at::Tensor stats, long R, long stride);
void conv_wgrad_stem_gemm_launch(at::Tensor x, at::Tensor dy, at::Tensor dw,
                                 long pad, long R, long stride);
