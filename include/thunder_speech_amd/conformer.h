/*
 * thunder_speech_amd/conformer.h -- companion C ABI of thunder_speech_amd.h: the conformer block of wav2vec2-conformer checkpoints with
 * rotary position embeddings.  The same shared library exports these entry points; the conventions are the core header's (DEVICE pointers
 * into caller-owned buffers, `stream` a hipStream_t passed as void*, 0 / TS_E* / positive hipError_t returns, nothing allocates, frees or
 * synchronises, so every call can be captured into a hipGraph).  The core ABI (TS_ABI_VERSION) and the WavLM companions are unchanged by
 * this header; it is versioned on its own by TS_CONFORMER_ABI_VERSION.
 *
 * Reference call site: huggingface/compatibility.py:31-42 (`self.original_encoder(audio, attention_mask=...)`) when the checkpoint is a
 * wav2vec2-conformer one -- transformers modeling_wav2vec2_conformer.py, Wav2Vec2ConformerEncoderLayer.forward.  Per layer (h: the f32
 * residual stream):
 *   h += 0.5 ffn1(LN(h));  h += attn(LN(h)) with q, k = linear(rot(LN(h))), v = linear(LN(h));  h += conv_module(h);  h += 0.5 ffn2(LN(h));
 *   h = LN(h);   conv_module(h) = pw2(act(BN(dwconv(GLU(pw1(LN(h)))))))
 * The feature front end, pw1, pw2, the attention core (ts_w2v_attention_fwd) and linear_out are the core header's launches.
 */
#ifndef THUNDER_SPEECH_AMD_CONFORMER_H
#define THUNDER_SPEECH_AMD_CONFORMER_H

#include <stdint.h>

#include "thunder_speech_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS_CONFORMER_ABI_VERSION 1

/* Version of this companion ABI (a binder checks it next to ts_abi_version). */
int ts_conformer_abi_version(void);

/* The convolution module between its two pointwise convolutions:
 *   y[b][f][j] = act(bn_scale[j] sum_i dw_w[i][j] g[b][f + i - (kernel - 1) / 2][j] + bn_shift[j]),  g[b][f][j] = u[b][f][j] sigmoid(u[b][f][c + j]),
 * g = 0 for frames outside [0, t) of clip b (the depthwise conv's zero padding; frames of the padded batch beyond a clip's length are
 * computed like any other frame, as transformers does).  u [B][t][2c] (pointwise_conv1's output), y [B][t][c]; dw_w f32 [kernel][c] (the
 * depthwise weight [c][1][kernel] transposed); bn_scale / bn_shift f32 [c]: the eval-mode BatchNorm folded on the host.  act 1: GELU (erf),
 * 2: SiLU.  precision 1: u and y bf16, arithmetic f32; precision 0: u and y f32.  One launch; GLU is evaluated once per staged element.
 * TS_EINVAL: a NULL pointer, batch or t or c <= 0.  TS_EUNSUPPORTED: an even kernel or kernel > 63, c % 8 != 0, u not 16-byte aligned,
 * act not 1 or 2, precision not 0 or 1, batch > 65535 (one grid row per clip). */
int ts_conformer_glu_dwconv_fwd(const void* u, int32_t batch, int32_t t, int32_t c, const float* dw_w, int32_t kernel, const float* bn_scale,
                                const float* bn_shift, int32_t act, int32_t precision, void* y, void* stream);

/* LayerNorm of the attention block and its rotated copy in one row pass: x f32 [B][t][c] ->
 *   y = LN(x) w + b  (what linear_v multiplies),   y_rot[j] = y[j] cos[p][j % 32] + s(j) y[j ^ 32] sin[p][j % 32]  per head of 64
 * (what linear_q and linear_k multiply), s(j) = -1 for j % 64 < 32, +1 otherwise (rotate_half), p = row % t: the frame within the padded
 * batch.  cos_sin f32 [2][t_table][32]: cos(p inv_freq) then sin(p inv_freq), built on the host (huggingface/conformer.py rotary_table).
 * precision 1: y and y_rot bf16; precision 0: f32.  TS_EINVAL: a NULL pointer, batch or t <= 0, t > t_table.  TS_EUNSUPPORTED: c != 64 heads,
 * c > 4096, precision not 0 or 1, x / w / b / cos_sin not 16-byte aligned, y / y_rot not 16-byte (precision 0) or 8-byte (precision 1)
 * aligned. */
int ts_conformer_layernorm_rotary_fwd(const float* x, const float* w, const float* b, float eps, int32_t batch, int32_t t, int32_t c, int32_t heads,
                                      const float* cos_sin, int32_t t_table, int32_t precision, void* y, void* y_rot, void* stream);

/* y[r][:n] = act(x[r][:k] W^T + bias) + res[r][:n]  with act 0: none, 1: GELU (erf), 2: SiLU.  W [n][k] (nn.Linear layout); bias / res f32
 * may be NULL; res == y with ld_res == ldc accumulates into y in place (the residual stream).  x: rows of pitch lda.
 * precision 1: x and W bf16 (w_frag: W as MFMA fragments from ts_gemm_nt_pack_w, or NULL); y f32 (pitch ldc) and / or y_op bf16 (pitch
 * ld_op) receive the result, either may be NULL -- y_op with ld_op = 3c lets the q|k and the v products write their column slices of one
 * [rows][3c] qkv buffer.  Shapes as ts_gemm_nt_bf16 (n % 32, k % 32, 16-byte aligned operands).
 * precision 0: x, W and y f32, y_op must be NULL; n % 4, ldc % 4, ld_res % 4 and 16-byte aligned y / res; res == y with act != 0 is
 *              TS_EUNSUPPORTED (the activation precedes the residual). */
int ts_conformer_linear_fwd(const void* x, int64_t lda, const void* w, const void* w_frag, const float* bias, const float* res, int64_t ld_res,
                            float* y, int64_t ldc, void* y_op, int64_t ld_op, int64_t rows, int32_t n, int32_t k, int32_t act, int32_t precision,
                            void* stream);

#ifdef __cplusplus
}
#endif

#endif /* THUNDER_SPEECH_AMD_CONFORMER_H */
