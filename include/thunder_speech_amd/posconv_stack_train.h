/*
 * thunder_speech_amd/posconv_stack_train.h -- companion C ABI of thunder_speech_amd.h: one layer of data2vec-audio's stacked positional
 * convolutions as a trainable node (csrc/posconv_stack_train.hip; the matrix-core conv is w2v_posconv_mfma_kernel of csrc/w2v_posconv.hip with
 * its raw-accumulator epilogue).  It is what fine-tuning a data2vec-audio checkpoint needs next to the launches of the core header.  The same
 * shared library exports these entry points; the conventions are the core header's (DEVICE pointers into caller-owned buffers, `stream` a
 * hipStream_t passed as void*, 0 / TS_E* / positive hipError_t returns, nothing allocates, frees or synchronises, so every call can be captured
 * into a hipGraph).  The core ABI (TS_ABI_VERSION) and the other companions are unchanged by this header; it is versioned on its own by
 * TS_POSCONV_STACK_TRAIN_ABI_VERSION.
 *
 * Reference call site: transformers' Data2VecAudioPositionalConvEmbedding (num_conv_pos_embeddings layers of Data2VecAudioPositionalConvLayer)
 * under the reference's training_step (src/thunder/module.py:102-127).  Per layer, on time-major f32 rows x [B][T][C]:
 *   z = grouped_conv1d(x, w, padding = k / 2)[..., :T]      (no bias here: it rides in the row kernel)
 *   n = (z + bias - mean_c) * rstd,  rstd = 1 / sqrt(var_c + eps)      nn.LayerNorm(elementwise_affine=False), eps 1e-5 (NOT config.layer_norm_eps)
 *   a = gelu(n)                                              erf form
 * The weight gradient of the conv is ts_w2v_posconv_wgrad of the core header, unchanged.
 */
#ifndef THUNDER_SPEECH_AMD_POSCONV_STACK_TRAIN_H
#define THUNDER_SPEECH_AMD_POSCONV_STACK_TRAIN_H

#include <stdint.h>

#include "../thunder_speech_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS_POSCONV_STACK_TRAIN_ABI_VERSION 1

/* Version of this companion ABI (a binder checks it next to ts_abi_version). */
int ts_posconv_stack_train_abi_version(void);

/* The grouped conv alone on the matrix cores: out [B][T][C] f32 = conv(src), bf16 operands, f32 accumulation, no bias, no activation, no
 * residual -- the raw-accumulator epilogue of the kernel behind ts_w2v_posconv_train, whose two epilogues are untouched.
 *   src [B][T][C] f32 (rounded to bf16 on the way into the padded copy);  w_taps_bf16 [kernel][groups][64 out][64 in] bf16.
 *   backward 0: out[b][s][g 64 + o] = sum_j sum_i src[b][s + j - kernel / 2][g 64 + i] w[j][g][o][i]   (kernel / 2 zero rows in front; an even kernel's
 *               extra last frame is never produced).
 *   backward 1: the data gradient, the same product with kernel - 1 - kernel / 2 zero rows in front; the caller passes the taps flipped and each
 *               tap's [out][in] block transposed (w_b[j] = w[kernel - 1 - j]^T), exactly as for ts_w2v_posconv_train(backward = 1), and nothing is added.
 * Rows outside [0, T) of a clip read as zero; clips do not see each other.
 * workspace: ts_posconv_stack_conv_workspace bytes, 16-byte aligned (the padded bf16 copy).  Two launches.
 * TS_EINVAL: a NULL pointer (the stream excepted); batch, t, c or groups <= 0; kernel <= 1; c % groups != 0.  TS_EUNSUPPORTED: c / groups != 64;
 * (128 + kernel - 1) * 144 > 64 KiB; src or workspace not 16-byte aligned.  The _workspace function returns a byte count, or TS_EINVAL (< 0)
 * for a non-positive argument. */
int64_t ts_posconv_stack_conv_workspace(int32_t batch, int32_t t, int32_t c, int32_t kernel);
int ts_posconv_stack_conv(const float* src, int32_t batch, int32_t t, int32_t c, const void* w_taps_bf16, int32_t kernel, int32_t groups,
                          int32_t backward, float* out, void* workspace, void* stream);

/* Forward row kernel: a [rows][c] f32 = gelu(LayerNorm_no_affine(z + bias; eps)), one pass over z (one wave per row, the row in registers), one
 * launch.  bias [c] f32.  Nothing is saved for the backward: it recomputes mean and rstd from z.
 * TS_EINVAL: a NULL pointer (the stream excepted); rows or c <= 0.  TS_EUNSUPPORTED: c % 4 != 0 or c > 4096; a pointer not 16-byte aligned. */
int ts_posconv_stack_norm_gelu_fwd(const float* z, const float* bias, float eps, int64_t rows, int32_t c, float* a, void* stream);

/* Backward row kernel, from z, bias and da [rows][c] f32 (mean, rstd and n are recomputed with the forward's arithmetic):
 *   dn = da gelu'(n);   dz [rows][c] = rstd (dn - mean_c(dn) - n mean_c(dn n));   dbias [c] = sum_rows dz.
 * dz is written once; dbias is WRITTEN (set, not added).  Two launches: the rows, each workgroup leaving the column sums of ITS rows in the
 * workspace, then the sum of those partials in a fixed order.  No atomics: equal arguments give equal bits.
 * workspace: ts_posconv_stack_norm_gelu_bwd_workspace bytes, 16-byte aligned.
 * TS_EINVAL: a NULL pointer (the stream excepted); rows or c <= 0.  TS_EUNSUPPORTED: as the forward.  The _workspace function returns a byte
 * count, or TS_EINVAL (< 0) for a non-positive argument. */
int64_t ts_posconv_stack_norm_gelu_bwd_workspace(int64_t rows, int32_t c);
int ts_posconv_stack_norm_gelu_bwd(const float* z, const float* bias, const float* da, float eps, int64_t rows, int32_t c, float* dz, float* dbias,
                                   void* workspace, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* THUNDER_SPEECH_AMD_POSCONV_STACK_TRAIN_H */
