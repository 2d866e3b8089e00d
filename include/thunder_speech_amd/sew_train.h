/*
 * thunder_speech_amd/sew_train.h -- companion C ABI of include/thunder_speech_amd.h: what fine-tuning a SEW encoder (transformers' SEWModel) in
 * mixed precision needs next to sew.h and the wav2vec2 training launches of the core header (csrc/sew_train.hip): the squeeze's forward that
 * keeps its pre-activation, its data gradient and its weight gradient, all on the matrix cores.  The same shared library exports these entry
 * points; the conventions are the core header's (DEVICE pointers into caller-owned buffers, `stream` a hipStream_t passed as void*,
 * 0 / TS_EINVAL / TS_EUNSUPPORTED / positive hipError_t returns, nothing allocates, frees or synchronises).  No atomics: equal arguments give equal
 * bits.  The core ABI, sew.h (TS_SEW_ABI_VERSION) and the other companions are unchanged by this header; it is versioned on its own by
 * TS_SEW_TRAIN_ABI_VERSION.
 *
 * Reference call site: the training-mode SEWEncoder.forward (transformers/models/sew/modeling_sew.py) under autograd, reached from the reference's
 * `BaseCTCModule.training_step` (src/thunder/module.py:102-127) through `_HuggingFaceEncoderAdapt.forward`.
 *
 * Notation: s = stride, k = kernel, p = k / 2, cg = c / groups, T2 = t / s (floor); x [B][t][c] f32 time-major; w the effective conv weight (weight
 * norm applied).  Support matrix of all three launches: cg 24 or 32 (24 is packed as 32 with zero lanes) and the forward's LDS condition -- exactly
 * the geometries ts_sew_squeeze_fwd(precision = 1) runs on its matrix-core kernel (huggingface/sew.py squeeze_on_matrix_cores); what that call
 * refuses with TS_EUNSUPPORTED (e.g. s = 3 with k = 128), and every other group width, these refuse too, before any launch.
 * TS_EINVAL of all three: a NULL pointer (the stream excepted); batch, t, c, kernel or groups <= 0; stride < 1; t < stride; c % groups != 0.
 * TS_EUNSUPPORTED: outside the support matrix; a pointer not 16-byte aligned (bias: 4-byte).
 * The two _workspace_bytes functions return a byte count, or TS_EINVAL (< 0) for a non-positive argument, stride < 1 or t < stride.
 */
#ifndef THUNDER_SPEECH_AMD_SEW_TRAIN_H
#define THUNDER_SPEECH_AMD_SEW_TRAIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TS_SEW_TRAIN_ABI_VERSION 1

/* Version of this companion ABI (a binder checks it next to ts_abi_version). */
int ts_sew_train_abi_version(void);

/* The geometry check the three launches below make behind their NULL checks and before anything else, on its own (no pointers, no launch): 0 when
 * they take the geometry, TS_EINVAL or TS_EUNSUPPORTED as they would return it. */
int ts_sew_squeeze_train_supported(int32_t batch, int32_t t, int32_t c, int32_t kernel, int32_t groups, int32_t stride);

/* ts_sew_squeeze_fwd(precision = 1) that also keeps the conv result: the same arguments, the same kernel and the same arithmetic -- y [B][T2][c] is
 * bit-equal to that call's -- plus z [B][T2][c] f32 = the accumulator before bias and GELU (what ts_w2v_posconv_train leaves for its backward).
 * w_taps: bf16 [k][groups][32 out][32 in] (pack_squeeze_taps).  workspace: ts_sew_squeeze_workspace_bytes(batch, t, c, kernel, stride, 1) bytes. */
int ts_sew_squeeze_train_fwd(const float* x, int32_t batch, int32_t t, int32_t c, const void* w_taps, const float* bias, int32_t kernel, int32_t groups,
                             int32_t stride, float* y, float* z, void* workspace, void* stream);

/* Data gradient of the squeeze, one kernel launch behind a padded bf16 copy of dz:
 *   dx[b][q][g cg + i] = pool^T(dy)[b][q][g cg + i] + sum_j sum_o dz[b][r][g cg + o] w[j][g][o][i]
 * over the taps j with (q + p - j) % s == 0 and r = (q + p - j) / s in [0, T2); pool^T(dy)[q] = dy[b][q / s] / s for q < s T2 and 0 for the rows
 * s T2 .. t - 1 (which still receive the conv term).  dz, dy [B][T2][c] f32; dx [B][t][c] f32, every element written.  bf16 operands (dz is rounded
 * on the way into the copy), f32 accumulation on the matrix cores; the pool term is added in f32 in the epilogue.
 * w_dgrad: bf16 [s][ceil(k / s)][groups][32 in][32 out], phase-major (pack_squeeze_dgrad_taps of huggingface/sew_train.py): block (f, u) is the
 * transposed tap j = f + s (ceil(k / s) - 1 - u) -- zeros where j >= k -- padded to 32 x 32.  The input rows with (q + p) % s == f are a stride-1
 * conv of dz with those taps; a workgroup stages one window of dz rows and produces the s phases from it.
 * workspace: ts_sew_squeeze_dgrad_workspace_bytes bytes, 16-byte aligned; contents are scratch. */
int64_t ts_sew_squeeze_dgrad_workspace_bytes(int32_t batch, int32_t t, int32_t c, int32_t kernel, int32_t stride);
int ts_sew_squeeze_dgrad(const float* dz, const float* dy, int32_t batch, int32_t t, int32_t c, const void* w_dgrad, int32_t kernel, int32_t groups,
                         int32_t stride, float* dx, void* workspace, void* stream);

/* Weight gradient of the squeeze's conv:
 *   dw[j][g][o][i] = sum_b sum_{r < T2} dz[b][r][g cg + o] x[b][s r + j - p][g cg + i],    frames outside [0, t) count as 0
 * dw f32 [k][groups][cg][cg] at the checkpoint's width (unpadded), written, not accumulated.  bf16 operands (both rounded on the way into padded
 * copies), f32 accumulation on the matrix cores: one workgroup per (block of 8 taps, pair of groups) contracts over all B T2 rows -- no partial
 * buffers.  workspace: ts_sew_squeeze_wgrad_workspace_bytes bytes, 16-byte aligned; contents are scratch. */
int64_t ts_sew_squeeze_wgrad_workspace_bytes(int32_t batch, int32_t t, int32_t c, int32_t kernel, int32_t stride);
int ts_sew_squeeze_wgrad(const float* dz, const float* x, int32_t batch, int32_t t, int32_t c, int32_t kernel, int32_t groups, int32_t stride, float* dw,
                         void* workspace, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* THUNDER_SPEECH_AMD_SEW_TRAIN_H */
