// What csrc/sew.hip (inference) and csrc/sew_train.hip (fine-tuning) share of SEW's squeeze on the matrix cores: the tile constants, the support
// condition of the matrix-core kernel, the padded bf16 copy and the forward launch (both defined in csrc/sew.hip, next to their kernels).
#pragma once
#include "ts_common.hpp"

namespace ts {

constexpr int SQ_TT = 128;         // output frames per workgroup
constexpr int SQ_PITCH = 144;      // bytes per staged row (64 bf16 + 16)
constexpr int SQ_SLOT = 32;        // channels per group in the padded copy and the packed weights
constexpr size_t SQ_LDS_MAX = 64 * 1024;

// rows per clip of the padded copies: t + kernel, rounded up to a multiple of the stride
static inline long long sew_prow(int t, int kernel, int stride) { return ((long long)t + kernel + stride - 1) / stride * stride; }

// whether sew_squeeze_mfma_kernel takes this geometry: 24 or 32 channels per group and the phase-split window within 64 KiB of LDS
static inline bool sew_squeeze_mfma_ok(int cg, int kernel, int stride) {
  if (cg != 24 && cg != SQ_SLOT) return false;
  const long long rows = (long long)(SQ_TT - 1) * stride + kernel, rpp = (rows + stride - 1) / stride;
  return (size_t)(stride * rpp) * SQ_PITCH <= SQ_LDS_MAX;
}

// bf16 copy of x [B][t][c] f32 as xp [B][prow][groups x 32]: `front` zero rows before each clip, zeros behind it and in channels c / groups .. 31 of each slot
void sew_pad16(hipStream_t stream, const float* x, unsigned short* xp, int batch, int t, int c, int groups, long long prow, int front);

// y = pool + gelu(conv + bias) on sew_squeeze_mfma_kernel behind its padded copy (workspace: ts_sew_squeeze_workspace_bytes); z: NULL, or [B][t / stride][c]
// for the conv result before bias and GELU.  The caller has checked the arguments and sew_squeeze_mfma_ok.
int sew_squeeze_mfma(hipStream_t stream, const float* x, int batch, int t, int c, const void* w_taps, const float* bias, int kernel, int groups, int stride,
                     float* y, float* z, void* workspace);

}  // namespace ts
