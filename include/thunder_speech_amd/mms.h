/*
 * thunder_speech_amd/mms.h -- companion C ABI of thunder_speech_amd.h: what the MMS checkpoints (facebook/mms-1b-all, -fl102, -l1107) and
 * XLS-R 1B need beyond the wav2vec2 launches -- the attention core at head_dim 80 and the per-layer attention adapter.  The same shared
 * library exports these entry points; the conventions are the core header's (DEVICE pointers into caller-owned buffers, `stream` a
 * hipStream_t passed as void*, 0 / TS_E* / positive hipError_t returns, nothing allocates, frees or synchronises, so every call can be
 * captured into a hipGraph).  The core ABI (TS_ABI_VERSION) and the other companions are unchanged by this header; it is versioned on its
 * own by TS_MMS_ABI_VERSION.
 *
 * Reference call site: huggingface/compatibility.py:31-42 (`self.original_encoder(audio, attention_mask=...)`) when the checkpoint sets
 * config.adapter_attn_dim -- transformers modeling_wav2vec2.py, Wav2Vec2EncoderLayerStableLayerNorm.forward (h: the f32 residual stream):
 *   h += attn(LN(h));  h += ffn(LN(h));  h += adapter_layer(h),   adapter_layer(h) = linear_2(relu(linear_1(LayerNorm(h; eps 1e-5))))
 * with hidden -> adapter_attn_dim -> hidden, and Wav2Vec2Attention at hidden 1280 / 16 heads.  Everything else of such a layer runs on the
 * core header's launches.
 */
#ifndef THUNDER_SPEECH_AMD_MMS_H
#define THUNDER_SPEECH_AMD_MMS_H

#include <stdint.h>

#include "thunder_speech_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS_MMS_ABI_VERSION 1

/* Version of this companion ABI (a binder checks it next to ts_abi_version). */
int ts_mms_abi_version(void);

/* Fused attention core at head_dim 80: ctx = softmax(q k^T / sqrt(80)) v per (clip, head), the [t][t] scores never stored -- no workspace.
 * qkv bf16 [B][t][3c] (q | k | v thirds of a row, head h = columns [80 h, 80 h + 80) of each), ctx bf16 [B][t][c].  key_len as
 * ts_w2v_attention_fwd: NULL = every key; key_len[b] <= 0 = all t keys; a value above t counts as t.  Scores and the softmax are f32, the
 * probabilities are rounded to bf16 for the second product (as ts_w2v_attention_fwd, precision 1).
 * TS_EINVAL: NULL qkv or ctx, batch / t / c / heads <= 0, c % heads != 0.  TS_EUNSUPPORTED: c / heads != 80, qkv or ctx not 16-byte
 * aligned, heads or batch > 65535 (grid dimensions). */
int ts_mms_attention_fwd(const void* qkv, int32_t batch, int32_t t, int32_t c, int32_t heads, const int32_t* key_len, void* ctx, void* stream);

/* The attention adapter, in place on the f32 residual stream h [rows][c], optionally with the LayerNorm that follows it in the same launch:
 *   h[r] += W2 relu(W1 LN(h[r]; norm_w, norm_b, eps 1e-5) + b1) + b2,     W1 [a][c], W2 [c][a] (nn.Linear layout), b1 [a], b2 [c]
 *   next_w != NULL:  LN(h[r]; next_w, next_b, next_eps) of the UPDATED row -> y_next (f32 [rows][c]) and / or y_next_op (bf16 [rows][c]);
 *                    either may be NULL, not both.  It is the next layer's layer_norm, or encoder.layer_norm after the last layer.
 * precision 0: w1 / w2 f32, every product on the f32 matrix-core instruction, y_next_op must be NULL.
 * precision 1: w1 / w2 bf16, LN(h) and relu(.) rounded to bf16 for the two products (f32 accumulation); the sum into h and both LayerNorms f32.
 * A workgroup holds 16 rows in registers and reads the weights once for all of them.
 * TS_EINVAL: NULL h / norm_w / norm_b / w1 / b1 / w2 / b2; rows, c or a <= 0; next_w without next_b; next_w with both outputs NULL.
 * TS_EUNSUPPORTED: a % 16 != 0 or a > 64; c % 8 != 0 or c > 4096 (the width ts_w2v_layernorm_fwd takes); precision not 0 or 1; y_next_op
 * with precision 0; a pointer not 16-byte aligned (y_next_op: 8-byte). */
int ts_mms_attn_adapter_fwd(float* h, int64_t rows, int32_t c, int32_t a, const float* norm_w, const float* norm_b, const void* w1, const float* b1,
                            const void* w2, const float* b2, const float* next_w, const float* next_b, float next_eps, float* y_next,
                            void* y_next_op, int32_t precision, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* THUNDER_SPEECH_AMD_MMS_H */
