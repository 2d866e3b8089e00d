/*
 * thunder_speech_amd/wavlm.h -- companion C ABI of thunder_speech_amd.h: the WavLM encoder's gated relative-position
 * attention.  The same shared library exports these entry points; the conventions are the core header's (DEVICE pointers
 * into caller-owned buffers, `stream` a hipStream_t passed as void*, 0 / TS_E* / positive hipError_t returns, nothing
 * allocates, frees or synchronises, so every call can be captured into a hipGraph).  The core ABI (TS_ABI_VERSION) is
 * unchanged by this header; it is versioned on its own by TS_WAVLM_ABI_VERSION.
 *
 * Reference call site: huggingface/compatibility.py:31-42 (`self.original_encoder(audio, attention_mask=...)`) when the
 * checkpoint is a WavLM one -- transformers modeling_wavlm.py, WavLMAttention.forward / compute_bias /
 * _relative_positions_bucket.  Everything else in a WavLM encoder layer is the wav2vec2 sequence of the core header
 * (ts_w2v_conv0_fwd ... ts_w2v_glu_fwd), with ts_wavlm_attention_fwd in place of ts_w2v_attention_fwd.
 */
#ifndef THUNDER_SPEECH_AMD_WAVLM_H
#define THUNDER_SPEECH_AMD_WAVLM_H

#include <stdint.h>

#include "thunder_speech_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS_WAVLM_ABI_VERSION 1

/* Version of this companion ABI (a binder checks it next to ts_abi_version). */
int ts_wavlm_abi_version(void);

/* Position-bias diagonals (compute_bias, evaluated once per forward in layer 0 and reused by every layer):
 *   rel_bias f32 [heads][2t - 1], rel_bias[h][d + t - 1] = embed[bucket(d)][h] for d = key - query in [-(t - 1), t - 1];
 *   bucket(d) = (d > 0) num_buckets / 2 + abs_bucket[min(|d|, max_distance)].
 * embed f32 [num_buckets][heads] (rel_attn_embed.weight of layer 0).  abs_bucket int32 [max_distance + 1]: the bucket of
 * -|d| (no sign offset) for 0 <= |d| <= max_distance, built on the host by the float32 restatement of
 * _relative_positions_bucket (huggingface/encoder.py wavlm_bucket_table) -- it does not depend on t; every |d| >= max_distance
 * lands in bucket num_buckets / 2 - 1.  One launch.  TS_EINVAL: a NULL pointer, num_buckets < 2, heads or t <= 0. */
int ts_wavlm_rel_bias(const float* embed, const int32_t* abs_bucket, int32_t num_buckets, int32_t max_distance, int32_t heads, int32_t t,
                      float* rel_bias, void* stream);

/* Gated relative-position self-attention core: qkv [B][t][3c] (q | k | v, heads are contiguous column blocks) ->
 *   ctx[b][i] = softmax_j(q_i k_j / sqrt(hd) + gate[b][h][i] rel_bias[h][j - i + t - 1] + key mask) v_j   per head h, hd = c / heads,
 *   p = gate_x[b][i][h hd .. h hd + hd - 1] gate_w^T + gate_b,  gate = sigmoid(p0 + p1 + p2 + p3) (sigmoid(p4 + p5 + p6 + p7) gate_const[h] - 1) + 2.
 * gate_x: the attention's INPUT rows (what the QKV projection multiplies: the layer input post-LN, the layer_norm output pre-LN),
 * row pitch ld_gate_x elements; gate_w f32 [8][hd] (gru_rel_pos_linear.weight), gate_b f32 [8], gate_const f32 [heads]
 * (gru_rel_pos_const), rel_bias from ts_wavlm_rel_bias.  key_len int32 [B] or NULL: keys >= key_len[b] get probability 0; a clip
 * with key_len <= 0 softmaxes over all t keys (the convention of ts_w2v_attention_fwd).
 * precision 0: qkv, gate_x and ctx f32; scores f32 in `workspace` (ts_wavlm_attention_workspace_bytes: B heads t t floats).
 * precision 1: qkv, gate_x and ctx bf16, hd must be 64 (fused MFMA kernel, no [t][t] matrix, no workspace: NULL is fine); gate_x
 *              and qkv 16-byte aligned, ld_gate_x a multiple of 8, else TS_EUNSUPPORTED. */
int64_t ts_wavlm_attention_workspace_bytes(int32_t batch, int32_t t, int32_t heads, int32_t precision);
int ts_wavlm_attention_fwd(const void* qkv, int32_t batch, int32_t t, int32_t c, int32_t heads, const int32_t* key_len, int32_t precision,
                           const void* gate_x, int64_t ld_gate_x, const float* gate_w, const float* gate_b, const float* gate_const,
                           const float* rel_bias, void* ctx, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* THUNDER_SPEECH_AMD_WAVLM_H */
