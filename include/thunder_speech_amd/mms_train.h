/*
 * thunder_speech_amd/mms_train.h -- companion C ABI of thunder_speech_amd.h: the fused attention core for mixed-precision FINE-TUNING at
 * head_dim 80 (XLS-R 1B / MMS geometry: hidden 1280, 16 heads), forward and backward (entry points in csrc/mms_train.hip, kernels in csrc/w2v_attn_train.hip).  The same shared library exports
 * these entry points; the conventions are the core header's (DEVICE pointers into caller-owned buffers, `stream` a hipStream_t passed as
 * void*, 0 / TS_E* / positive hipError_t returns, nothing allocates, frees or synchronises, so every call can be captured into a hipGraph).
 * The core ABI (TS_ABI_VERSION) and the other companions are unchanged by this header; it is versioned on its own by TS_MMS_TRAIN_ABI_VERSION.
 *
 * Reference call site: transformers' Wav2Vec2Attention inside the checkpoint's encoder under the reference's training_step (thunder
 * module.py:102-127, huggingface/compatibility.py:31-42): ctx = dropout(softmax(q k^T / sqrt(80) + key mask)) v.  The contract is that of
 * ts_w2v_attention_train_fwd / _bwd (thunder_speech_amd.h) at head_dim 80; training the MMS attention adapters is not part of it.
 */
#ifndef THUNDER_SPEECH_AMD_MMS_TRAIN_H
#define THUNDER_SPEECH_AMD_MMS_TRAIN_H

#include <stdint.h>

#include "thunder_speech_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS_MMS_TRAIN_ABI_VERSION 1

/* Version of this companion ABI (a binder checks it next to ts_abi_version). */
int ts_mms_train_abi_version(void);

/* No [t][t] score / probability matrix exists in either direction.
 *   ts_mms_attention_train_fwd   ctx = dropout(softmax(q k^T / sqrt(80) + key mask)) v;  qkv bf16 [B][t][3c] (q | k | v thirds of a row, head h =
 *                                columns [80 h, 80 h + 80) of each), ctx f32 [B][t][c], lse2 f32 [B][heads][t] = the row statistic max + log2(sum)
 *                                in the log2 domain (scale folded in) the backward rebuilds probabilities from; +inf for a row with no valid key.
 *                                Dropout: the mask of ts_train_dropout over the logical [B * heads * t][t] probability matrix (element
 *                                e = row * t + key: word e & 3 of Philox block e >> 2 under `seed`), kept entries scaled by 1 / (1 - p_drop); drawn
 *                                once per call as a bitstring into `workspace` (ts_mms_attention_train_fwd_workspace bytes; unused and may be
 *                                NULL when p_drop = 0).
 *   ts_mms_attention_train_bwd   dqkv f32 [B][t][3c] (every element written) from dctx f32 [B][t][c], ctx, lse2 and the same qkv / key_len /
 *                                p_drop / seed;  fwd_mask: the forward call's workspace if the caller kept it, else NULL (the mask is then
 *                                re-drawn from the seed, same bits);  workspace: ts_mms_attention_train_bwd_workspace bytes, laid out as the bf16
 *                                copy of dctx, then the row sums D f32 [B][heads][t], then room for the mask bits.  Four launches at most (mask,
 *                                row sums, dQ, dK / dV); the last two each rebuild the probabilities: no atomics, fixed summation order, so equal
 *                                arguments give equal bits.
 * key_len int32 [B] or NULL = every key; keys >= key_len[b] get probability 0; key_len[b] <= 0 (no valid key): every probability of the clip is
 * 0, ctx = 0 and all three gradients 0 (ts_w2v_softmax_fwd's convention, NOT ts_mms_attention_fwd's); a value above t counts as t.
 * Operands bf16 (q, k, v, dctx, the probabilities and their gradient), softmax, accumulation and results f32.
 * TS_EINVAL: a NULL required pointer (qkv, ctx, lse2, dctx, dqkv, the backward's workspace, the forward's when p_drop > 0); batch, t, c or
 * heads <= 0; c % heads != 0; p_drop outside [0, 1).  TS_EUNSUPPORTED: c / heads != 80; a pointer not 16-byte aligned;
 * batch * heads * t * t >= 2^40; heads or batch > 65535 (grid dimensions).  The _workspace functions return a byte count, or TS_EINVAL (< 0)
 * for a non-positive argument. */
int64_t ts_mms_attention_train_fwd_workspace(int32_t batch, int32_t t, int32_t c, int32_t heads);
int ts_mms_attention_train_fwd(const void* qkv_bf16, int32_t batch, int32_t t, int32_t c, int32_t heads, const int32_t* key_len, float p_drop,
                               uint64_t seed, float* ctx, float* lse2, void* workspace, void* stream);
int64_t ts_mms_attention_train_bwd_workspace(int32_t batch, int32_t t, int32_t c, int32_t heads);
int ts_mms_attention_train_bwd(const void* qkv_bf16, int32_t batch, int32_t t, int32_t c, int32_t heads, const int32_t* key_len, float p_drop,
                               uint64_t seed, const float* dctx, const float* ctx, const float* lse2, const void* fwd_mask, float* dqkv,
                               void* workspace, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* THUNDER_SPEECH_AMD_MMS_TRAIN_H */
