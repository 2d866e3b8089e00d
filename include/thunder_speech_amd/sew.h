/*
 * thunder_speech_amd/sew.h -- companion C ABI of include/thunder_speech_amd.h: the two launches a SEW encoder (transformers' SEWModel, the
 * "squeezed and efficient" wav2vec2) needs next to the wav2vec2 launches of the core header (csrc/sew.hip).  The same shared library exports these
 * entry points; the conventions are the core header's (DEVICE pointers into caller-owned buffers, `stream` a hipStream_t passed as void*,
 * 0 / TS_EINVAL / TS_EUNSUPPORTED / positive hipError_t returns, nothing allocates, frees or synchronises, so every call can be captured into a
 * hipGraph).  The core ABI (TS_ABI_VERSION) and the other companions are unchanged by this header; it is versioned on its own by
 * TS_SEW_ABI_VERSION.
 *
 * Reference call site: SEWEncoder.forward (transformers/models/sew/modeling_sew.py), reached from the reference's
 * `_HuggingFaceEncoderAdapt.forward` (src/thunder/huggingface/compatibility.py:31-42) for a SEW checkpoint:
 *   squeeze    hidden = AvgPool1d(s, s)(h) + gelu(same_pad(weight_normed grouped Conv1d(stride = s, padding = k / 2)(h)))     [B][T / s][C]
 *   upsample   gelu(Linear(C -> s C)(hidden)) read row-major as [B][s (T / s)][C], zero rows up to T
 */
#ifndef THUNDER_SPEECH_AMD_SEW_H
#define THUNDER_SPEECH_AMD_SEW_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TS_SEW_ABI_VERSION 1

/* Version of this companion ABI (a binder checks it next to ts_abi_version). */
int ts_sew_abi_version(void);

/* The squeeze in one call, on time-major f32 rows x [B][T][C]; T2 = T / stride (floor), for r < T2:
 *   y[b][r][c] = mean_{i < stride} x[b][stride r + i][c]
 *              + gelu(bias[c] + sum_j sum_ci w[j][g][o][ci] x[b][stride r + j - kernel / 2][g cg + ci]),    c = g cg + o, cg = C / groups
 * x reads as zero outside [0, T); clips do not see each other; the GELU is the erf form; y [B][T2][C] f32.
 *   precision 1 with cg 24 or 32: bf16 operands (x is rounded on the way into the padded copy), f32 accumulation on the matrix cores, one
 *     kernel launch behind the padded copy; the average pool reads the f32 x.  w_taps is bf16 [kernel][groups][32 out][32 in]: with cg = 24
 *     each block is padded to 32 x 32 with zeros (rows and columns 24 .. 31).
 *   precision 0, or any other cg in either precision: f32 operands and f32 accumulation (the library's f32 GEMM over a padded f32 copy, then
 *     a row kernel).  w_taps is f32 [kernel][groups][cg out][cg in].
 * No atomics: equal arguments give equal bits.
 * workspace: ts_sew_squeeze_workspace_bytes bytes, 16-byte aligned (the padded copy, and the f32 path's conv result); contents are scratch.
 * TS_EINVAL: a NULL pointer (the stream excepted); batch, t, c, kernel or groups <= 0; stride < 1; t < stride; c % groups != 0.
 * TS_EUNSUPPORTED: precision outside {0, 1}; x, w_taps, y or workspace not 16-byte aligned, bias not 4-byte aligned; on the
 * matrix-core path a window of (127 stride + kernel) rows x 144 bytes (rounded up to a multiple of stride rows) over 64 KiB of LDS.
 * The _workspace function returns a byte count that serves either path of the given shape, or TS_EINVAL (< 0) for a non-positive argument,
 * stride < 1 or t < stride, or TS_EUNSUPPORTED for a precision outside {0, 1}. */
int64_t ts_sew_squeeze_workspace_bytes(int32_t batch, int32_t t, int32_t c, int32_t kernel, int32_t stride, int32_t precision);
int ts_sew_squeeze_fwd(const float* x, int32_t batch, int32_t t, int32_t c, const void* w_taps, const float* bias, int32_t kernel, int32_t groups,
                       int32_t stride, int32_t precision, float* y, void* workspace, void* stream);

/* The upsampler's row layout when T is no multiple of stride: src [B][t2][stride c] f32 (the GELU of the upsampling projection) is, row-major,
 * [B][stride t2][c]; dst [B][t][c] f32 gets those rows and zero rows stride t2 .. t - 1.  (With t == stride t2 the source already is the result
 * and no call is needed.)  One launch of 16-byte copies.
 * TS_EINVAL: a NULL pointer (the stream excepted); batch, t2 or c <= 0; stride < 1; t < stride t2.
 * TS_EUNSUPPORTED: c % 4 != 0; src or dst not 16-byte aligned. */
int ts_sew_unsqueeze_rows(const float* src, int32_t batch, int32_t t2, int32_t t, int32_t c, int32_t stride, float* dst, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* THUNDER_SPEECH_AMD_SEW_H */
