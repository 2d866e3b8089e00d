/*
 * thunder_speech_amd/wavlm_train.h -- second companion C ABI of thunder_speech_amd.h: mixed-precision FINE-TUNING of the WavLM
 * encoder's gated relative-position attention (forward and backward without a [t][t] buffer, the gate and the position-bias
 * embedding with their gradients).  The same shared library exports these entry points; the conventions are the core header's
 * (DEVICE pointers into caller-owned buffers, `stream` a hipStream_t passed as void*, 0 / TS_E* / positive hipError_t returns,
 * nothing allocates, frees or synchronises, so every call can be captured into a hipGraph; no float atomics, so two calls give
 * the same bits).  Neither the core ABI (TS_ABI_VERSION) nor the WavLM inference ABI (TS_WAVLM_ABI_VERSION) changes with this
 * header; it is versioned on its own by TS_WAVLM_TRAIN_ABI_VERSION.
 *
 * Reference call site: huggingface/compatibility.py:31-42 (`self.original_encoder(audio, attention_mask=...)`) in train mode under
 * BaseCTCModule.training_step (module.py:102-127) when the checkpoint is a WavLM one -- transformers modeling_wavlm.py,
 * WavLMAttention.forward (gate, gated_position_bias, F.multi_head_attention_forward with dropout), compute_bias, and
 * WavLMEncoder / WavLMEncoderStableLayerNorm.forward (layer 0's position bias passed to every layer).
 * Shapes: B clips, t frames, heads H, c = 64 H channels; the gate and its gradient are f32 [B][H][t], the position-bias
 * diagonals rel_bias f32 [H][2t - 1] with rel_bias[h][d + t - 1] the bias of key - query = d (ts_wavlm_rel_bias).
 */
#ifndef THUNDER_SPEECH_AMD_WAVLM_TRAIN_H
#define THUNDER_SPEECH_AMD_WAVLM_TRAIN_H

#include <stdint.h>

#include "thunder_speech_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS_WAVLM_TRAIN_ABI_VERSION 1

/* Version of this companion ABI (a binder checks it next to ts_abi_version and ts_wavlm_abi_version). */
int ts_wavlm_train_abi_version(void);

/* Gate of WavLMAttention.forward steps 1-3 (gru_rel_pos_linear, the (2, 4) sums, sigmoid, gru_rel_pos_const):
 *   p = x[b][i][64 h .. 64 h + 63] gate_w^T + gate_b,  ga = sigmoid(p0 + p1 + p2 + p3),  gb = sigmoid(p4 + p5 + p6 + p7),
 *   gate[b][h][i] = ga (gb gate_const[h] - 1) + 2.
 * x f32 [B][t][ld_x] (the attention's INPUT rows: the layer input post-LN, the layer_norm output pre-LN), gate_w f32 [8][64],
 * gate_b f32 [8], gate_const f32 [heads].  gate_ab f32 [2][B][H][t] receives ga then gb for ts_wavlm_gate_bwd.
 * TS_EINVAL: a NULL pointer, batch / t / heads <= 0, ld_x < 64 heads.  TS_EUNSUPPORTED: x not 16-byte aligned or ld_x % 4. */
int ts_wavlm_gate_fwd(const float* x, int32_t batch, int32_t t, int32_t heads, int64_t ld_x, const float* gate_w, const float* gate_b,
                      const float* gate_const, float* gate, float* gate_ab, void* stream);

/* Backward of ts_wavlm_gate_fwd for the gate gradient dgate f32 [B][H][t]:
 *   dp0..3 = dgate (gb c - 1) ga (1 - ga),  dp4..7 = dgate ga c gb (1 - gb),
 *   dx[b][i][64 h + d] = sum_r dp_r gate_w[r][d]  (WRITTEN, columns [0, 64 heads) of each row of pitch ld_x),
 *   dgate_w[r][d] = sum dp_r x_h[d],  dgate_b[r] = sum dp_r,  dgate_const[h] = sum_{b,i} dgate ga gb  (all written, fixed summation order).
 * workspace: ts_wavlm_gate_bwd_workspace bytes (per-wave partials).  Two launches. */
int64_t ts_wavlm_gate_bwd_workspace(int32_t batch, int32_t t, int32_t heads);
int ts_wavlm_gate_bwd(const float* x, int32_t batch, int32_t t, int32_t heads, int64_t ld_x, const float* gate_w, const float* gate_const,
                      const float* gate_ab, const float* dgate, float* dx, float* dgate_w, float* dgate_b, float* dgate_const, void* workspace,
                      void* stream);

/* Training forward of the attention core (torch_multi_head_self_attention in train mode, head_dim 64): for clip b, head h, query i, key j
 *   s_ij = q_i k_j / 8 + gate[b][h][i] rel_bias[h][j - i + t - 1],  keys j >= key_len[b] get probability 0,
 *   ctx_i = sum_j dropout(softmax_j(s_i))_ij v_j,
 * the arguments of ts_w2v_attention_train_fwd plus `gate` (ts_wavlm_gate_fwd) and `rel_bias` (ts_wavlm_rel_bias).  qkv bf16
 * [B][t][3c] 16-byte aligned, ctx f32 [B][t][c], lse2 f32 [B][H][t] (log2-domain row statistic, bias included, for the backward).
 * Dropout: the mask is ts_train_dropout's for `seed` over the logical [B H t][t] matrix (the same stream as ts_w2v_attention_train_fwd),
 * drawn once into `workspace` (ts_wavlm_attention_train_fwd_workspace bytes; NULL allowed when p_drop == 0).  A clip with key_len <= 0
 * gets ctx = 0 (and zero gradients).  TS_EUNSUPPORTED: head_dim != 64, misalignment. */
int64_t ts_wavlm_attention_train_fwd_workspace(int32_t batch, int32_t t, int32_t c, int32_t heads);
int ts_wavlm_attention_train_fwd(const void* qkv_bf16, int32_t batch, int32_t t, int32_t c, int32_t heads, const int32_t* key_len, float p_drop,
                                 uint64_t seed, const float* gate, const float* rel_bias, float* ctx, float* lse2, void* workspace, void* stream);

/* Backward of ts_wavlm_attention_train_fwd for dctx f32 [B][t][c] (ctx, lse2 from the forward; fwd_mask = the forward's workspace,
 * or NULL to redraw the mask from the seed): with dS = P (dP - D) the gradient of the logits,
 *   dqkv f32 [B][t][3c]  (dq = dS k / 8, dk = dS^T q / 8, dv = P_d^T dctx; every element written),
 *   dgate f32 [B][H][t]  dgate[b][h][i] = sum_j dS_ij rel_bias[h][j - i + t - 1],
 *   drel_bias f32 [H][2t - 1]  drel_bias[h][d + t - 1] = sum_b sum_i gate[b][h][i] dS[b][h][i][i + d]  (this call's layer only).
 * workspace: ts_wavlm_attention_train_bwd_workspace bytes, 16-byte aligned (bf16 dctx, row dots, per-(clip, head, 64-key tile,
 * 32-query tile) diagonal partials of drel_bias summed in a fixed order, the redrawn mask).  Five launches at most. */
int64_t ts_wavlm_attention_train_bwd_workspace(int32_t batch, int32_t t, int32_t c, int32_t heads);
int ts_wavlm_attention_train_bwd(const void* qkv_bf16, int32_t batch, int32_t t, int32_t c, int32_t heads, const int32_t* key_len, float p_drop,
                                 uint64_t seed, const float* gate, const float* rel_bias, const float* dctx, const float* ctx, const float* lse2,
                                 const void* fwd_mask, float* dqkv, float* dgate, float* drel_bias, void* workspace, void* stream);

/* Gradient of ts_wavlm_rel_bias (compute_bias's rel_attn_embed lookup): dembed[k][h] = sum of drel_bias[h][d + t - 1] over the
 * diagonals d in [-(t - 1), t - 1] whose bucket (the same abs_bucket rule as ts_wavlm_rel_bias) is k; a bucket no diagonal maps to
 * gets 0.  dembed f32 [num_buckets][heads], every element written.  One launch, a gather per (bucket, head). */
int ts_wavlm_rel_bias_bwd(const float* drel_bias, const int32_t* abs_bucket, int32_t num_buckets, int32_t max_distance, int32_t heads, int32_t t,
                          float* dembed, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* THUNDER_SPEECH_AMD_WAVLM_TRAIN_H */
