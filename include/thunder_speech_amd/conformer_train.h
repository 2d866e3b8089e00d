/*
 * thunder_speech_amd/conformer_train.h -- companion C ABI of include/thunder_speech_amd.h: what mixed-precision FINE-TUNING of a rotary
 * wav2vec2-conformer needs beyond the wav2vec2 training kernels (csrc/conformer_train.hip; the Python chain is huggingface/conformer_train.py):
 * the convolution module between its two pointwise products with BatchNorm on batch statistics, forward and backward, the transpose of the
 * rotary rotation, and the feed-forward activation pair with an activation code.  The same shared library exports these entry points; the
 * conventions are the core header's (DEVICE pointers into caller-owned buffers, `stream` a hipStream_t passed as void*, 0 / TS_EINVAL /
 * TS_EUNSUPPORTED / positive hipError_t returns, workspace sizes from the *_workspace queries, nothing allocates, frees or synchronises,
 * argument checks before any launch).  The core ABI (TS_ABI_VERSION) and the other companions are unchanged by this header; it is versioned on
 * its own by TS_CONFORMER_TRAIN_ABI_VERSION.
 *
 * transformers call sites (modeling_wav2vec2_conformer.py, train mode): Wav2Vec2ConformerConvolutionModule.forward (glu, depthwise_conv,
 * batch_norm, activation), Wav2Vec2ConformerSelfAttention._apply_rotary_embedding, Wav2Vec2ConformerFeedForward.forward (intermediate_act_fn,
 * intermediate_dropout), each with its autograd backward.
 *
 * Activations are time-major f32 [B][t][c]; bf16 exists only as GEMM operands.  Notation: k the odd depthwise kernel, P = (k - 1) / 2,
 * G[b][f][j] = u[b][f][j] sigmoid(u[b][f][c + j]) (0 for f outside [0, t)), n = B t, zh = (z - mean) rstd, y = gamma zh + beta.  Frames of the
 * padded batch beyond a clip's length are ordinary frames, as in transformers.  act: 1 = GELU (erf), 2 = SiLU.  dw_w is [k][c] (tap-major).
 * No kernel here uses an atomic and every reduction has a fixed order: equal arguments give equal bits.
 *
 * Common refusals.  TS_EINVAL: a NULL pointer (the stream excepted), batch, t, c or rows <= 0.  TS_EUNSUPPORTED: an even kernel or one outside
 * [1, 63], c % 8 != 0 (c % 64 != 0 for ts_conformer_rotary_bwd), act not 1 or 2, a pointer that is not 16-byte aligned, batch > 65535.
 * TS_EINVAL is checked first.
 */
#ifndef THUNDER_SPEECH_AMD_CONFORMER_TRAIN_H
#define THUNDER_SPEECH_AMD_CONFORMER_TRAIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TS_CONFORMER_TRAIN_ABI_VERSION 1

/* Version of this companion ABI (a binder checks it next to ts_abi_version). */
int ts_conformer_train_abi_version(void);

/* z[b][f][j] = sum_i dw_w[i][j] G[b][f + i - P][j], f32 [B][t][c], NOT normalised: a workgroup stages 128 GLU'd frames and their halo of 64
 * channels in LDS (the layout of ts_conformer_glu_dwconv_fwd).  The same launch writes, per workgroup and channel, (count, mean, centred sum of
 * squares) of its z into the workspace (float64; summed in float64 in a fixed order).
 * Workspace bytes: batch ceil(t / 128) 3 c 8 -- the query returns TS_EINVAL (< 0) for batch, t or c <= 0. */
int64_t ts_conformer_glu_dwconv_train_fwd_workspace(int32_t batch, int32_t t, int32_t c);
int ts_conformer_glu_dwconv_train_fwd(const float* u, int32_t batch, int32_t t, int32_t c, const float* dw_w, int32_t kernel, float* z,
                                      void* workspace, void* stream);

/* Batch statistics of z over all n = batch t frames from the partials ts_conformer_glu_dwconv_train_fwd left in `workspace` (same batch, t, c),
 * combined in float64 in workgroup order by Chan's formula:  mean_rstd f32 [2][c] = (mean, 1 / sqrt(var_biased + eps)),  mean_var f32 [2][c] =
 * (mean, var_biased) for the running update.  TS_EINVAL also for n < 2 (torch refuses one value per channel in train mode). */
int ts_conformer_bn_stats(const void* workspace, int32_t batch, int32_t t, int32_t c, float eps, float* mean_rstd, float* mean_var, void* stream);

/* a = act(gamma (z - mean) rstd + beta) written straight as the bf16 operand y_bf16 [rows][c] of pointwise_conv2 and / or its transposed copy
 * yt_bf16 [c][rows_pad] (pitch ldt; rows >= `rows` zero), the contract of ts_w2v_ffn_act_cast: the f32 activation is never stored.  With running
 * statistics the caller passes (running_mean, 1 / sqrt(running_var + eps)) as mean_rstd.  TS_EINVAL also for both outputs NULL, rows >= 2^31,
 * rows_pad < rows or ldt < rows_pad; TS_EUNSUPPORTED also for an odd ldt. */
int ts_conformer_bn_act_cast(const float* z, const float* mean_rstd, const float* gamma, const float* beta, int64_t rows, int32_t c, int32_t act,
                             void* y_bf16, void* yt_bf16, int64_t ldt, int64_t rows_pad, void* stream);

/* With g = da act'(y) (da: the f32 data gradient of pointwise_conv2):  dbeta[j] = sum_rows g,  dgamma[j] = sum_rows g zh, f32 [c] each, WRITTEN:
 * partials per 32 rows in the workspace, then an ordered float64 finish.  Workspace bytes: ceil(rows / 32) 2 c 4; TS_EUNSUPPORTED also for rows > 32 x 65535. */
int64_t ts_conformer_bn_act_bwd_sums_workspace(int64_t rows, int32_t c);
int ts_conformer_bn_act_bwd_sums(const float* z, const float* mean_rstd, const float* gamma, const float* beta, const float* da, int64_t rows,
                                 int32_t c, int32_t act, float* dgamma, float* dbeta, void* workspace, void* stream);

/* The backward of activation, BatchNorm, depthwise conv and GLU in one launch plus an ordered finish of the weight gradient.  It recomputes g,
 * forms  dz = gamma rstd (g - dbeta / n - zh dgamma / n)  (running_stats != 0:  dz = gamma rstd g, dgamma / dbeta are not read for it) for a
 * tile's frames and halo in LDS -- dz never goes to memory -- and from that one staged tile takes both
 *   dG[b][f][j] = sum_i dw_w[i][j] dz[b][f - i + P][j]   ->   du[b][f][j] = dG s,  du[b][f][c + j] = dG u1 s (1 - s),  s = sigmoid(u[b][f][c + j])
 *   d_dw[i][j]  = sum_{b, f} dz[b][f - i + P][j] G[b][f][j]      (= sum dz[b][f][j] G[b][f + i - P][j])
 * du f32 [B][t][2c], d_dw f32 [k][c], both WRITTEN.  dgamma / dbeta: the results of ts_conformer_bn_act_bwd_sums for the same arguments.
 * Workspace bytes: batch ceil(t / 128) kernel c 4.  TS_EINVAL also for n < 2 with batch statistics. */
int64_t ts_conformer_glu_dwconv_train_bwd_workspace(int32_t batch, int32_t t, int32_t c, int32_t kernel);
int ts_conformer_glu_dwconv_train_bwd(const float* u, const float* z, const float* da, int32_t batch, int32_t t, int32_t c, const float* dw_w,
                                      int32_t kernel, const float* mean_rstd, const float* gamma, const float* beta, const float* dgamma,
                                      const float* dbeta, int32_t running_stats, int32_t act, float* du, float* d_dw, void* workspace, void* stream);

/* The transpose of the rotation of ts_conformer_layernorm_rotary_fwd added to the value branch's gradient (rows = batch t, position p = row % t,
 * cos_sin f32 [2][t_table][32] as there):
 *   dy[j] = dy_v[j] + dy_rot[j] cos[p][j % 32] - s(j) dy_rot[j ^ 32] sin[p][j % 32],   s(j) = -1 for j % 64 < 32, else +1.
 * dy feeds ts_w2v_layernorm_bwd_set.  TS_EINVAL also for t > t_table. */
int ts_conformer_rotary_bwd(const float* dy_v, const float* dy_rot, int32_t batch, int32_t t, int32_t c, const float* cos_sin, int32_t t_table,
                            float* dy, void* stream);

/* ts_w2v_ffn_act_cast / ts_w2v_ffn_act_bwd with an activation code: y16 = bf16(dropout(act(z + bias))) (+ the transposed copy), and
 * dz = dropout_backward(da) act'(z + bias); the mask is ts_train_dropout's under `seed`.  act 1 runs the wav2vec2 pair itself (the same bits);
 * bias may be NULL; c % 4 == 0 suffices here.  Refusals as that pair's. */
int ts_conformer_ffn_act_cast(const float* z, const float* bias, int64_t rows, int32_t c, int32_t act, float p_drop, uint64_t seed, void* y_bf16,
                              void* yt_bf16, int64_t ldt, int64_t rows_pad, void* stream);
int ts_conformer_ffn_act_bwd(const float* z, const float* bias, int32_t c, int32_t act, const float* da, float p_drop, uint64_t seed, float* dz,
                             int64_t n, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* THUNDER_SPEECH_AMD_CONFORMER_TRAIN_H */
