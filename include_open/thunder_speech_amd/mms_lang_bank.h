/*
 * thunder_speech_amd/mms_lang_bank.h -- companion C ABI of thunder_speech_amd.h: many MMS languages served on one frozen base
 * (csrc/mms_lang_bank.hip).  An MMS checkpoint (facebook/mms-1b-all and its kin) is one base plus, per language, the attention adapters of
 * every layer and a CTC head on that language's vocabulary.  Here both come from banks, and every clip of a batch picks its language by a
 * slot id read on the device at run time: one packed base, many languages, one captured graph whatever the mix of languages in the batch.
 * The same shared library exports these entry points; the conventions are the core header's (DEVICE pointers into caller-owned buffers,
 * `stream` a hipStream_t passed as void*, 0 / TS_E* / positive hipError_t returns, nothing allocates, frees or synchronises, so every call
 * can be captured into a hipGraph).  It is versioned on its own by TS_MMS_LANG_BANK_ABI_VERSION.
 *
 * Both launches read ids, int32 [batch] on the device: clip b is served by slot ids[b]; an id outside [0, n_slots) is served by SLOT 0,
 * which by the caller's convention holds the language the checkpoint was loaded with (-1 selects it; a stale id cannot cause a read
 * outside the banks).  The id is read at run time: a replayed graph serves what ids holds at replay.  A clip's result depends on nothing
 * outside that clip; no atomics, a fixed summation order: equal arguments give equal bits.
 *
 * No reference call site: the reference loads one language per module (huggingface/compatibility.py:45-112 through transformers'
 * target_lang).  The arithmetic of the adapter launch is ts_mms_attn_adapter_fwd's (thunder_speech_amd/mms.h), bit for bit.
 *
 * Out of scope: training with a bank; banks on the conformer, SEW and WavLM plans; a bank under precision="mxfp8"; LM fusion, alignment and
 * long-form transcription under a mixed-language selection; languages whose blank index differs from the resident one's; downloading
 * language packs; folding the head into the last adapter launch.
 */
#ifndef THUNDER_SPEECH_AMD_MMS_LANG_BANK_H
#define THUNDER_SPEECH_AMD_MMS_LANG_BANK_H

#include <stdint.h>

#include "thunder_speech_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS_MMS_LANG_BANK_ABI_VERSION 1

/* Version of this companion ABI (a binder checks it next to ts_abi_version). */
int ts_mms_lang_bank_abi_version(void);

/* ts_mms_attn_adapter_fwd with the six adapter tensors of ONE layer taken from banks, each clip with the tensors of its own slot:
 *   h [batch][t][c] f32, updated in place:  h[b][r] += W2_s relu(W1_s LN(h[b][r]; norm_w_s, norm_b_s, eps 1e-5) + b1_s) + b2_s,  s = slot of b
 *   norm_w, norm_b [n_slots][c] f32;  w1 [n_slots][a][c], w2 [n_slots][c][a]: f32 (precision 0) or bf16 (precision 1);  b1 [n_slots][a],
 *   b2 [n_slots][c] f32
 *   next_w != NULL:  LN(h[b][r]; next_w, next_b, next_eps) of the UPDATED row -> y_next (f32 [batch][t][c]) and / or y_next_op (bf16), as
 *                    ts_mms_attn_adapter_fwd; next_w / next_b [c] are the base's and shared by every slot.
 * A workgroup holds 16 rows of ONE clip (a clip's last tile is partial when t % 16 != 0) and reads its slot once.  Every row's arithmetic is
 * ts_mms_attn_adapter_fwd's in the same order: h, y_next and y_next_op of clip b equal, bit for bit, what that launch writes for the clip's
 * t rows alone with slot s's tensors.
 * TS_EINVAL: what ts_mms_attn_adapter_fwd returns it for (NULL h / norm_w / norm_b / w1 / b1 / w2 / b2; c or a <= 0; next_w without next_b;
 * next_w with both outputs NULL), and n_slots <= 0, NULL ids, batch or t <= 0.  TS_EUNSUPPORTED: what ts_mms_attn_adapter_fwd returns it
 * for (a % 16 != 0 or a > 64; c % 8 != 0 or c > 4096; precision not 0 or 1; y_next_op with precision 0; a pointer not 16-byte aligned,
 * y_next_op: 8-byte), ids not 4-byte aligned, and batch > 65535 (a grid dimension). */
int ts_mms_lang_bank_adapter_fwd(float* h, int32_t batch, int32_t t, int32_t c, int32_t a, const float* norm_w, const float* norm_b, const void* w1,
                                 const float* b1, const void* w2, const float* b2, int32_t n_slots, const int32_t* ids, const float* next_w,
                                 const float* next_b, float next_eps, float* y_next, void* y_next_op, int32_t precision, void* stream);

/* The CTC head per clip, on the encoder's time-major output, written class-major as the decoders take it:
 *   logits[b][v][f] = bias_bank[s][v] + sum_k w_bank[s][v][k] h[b][f][k]     for v < vocab[s],     -1e30f for vocab[s] <= v < v_pad
 *   h f32 [batch][t][c];  w_bank [n_slots][v_pad][c]: bf16 (precision 1) or f32 (precision 0);  bias_bank f32 [n_slots][v_pad];
 *   vocab int32 [n_slots] on the device: the classes of the language in the slot (a value above v_pad counts as v_pad);
 *   logits f32 [batch][v_pad][ldt]: columns f < t of every row are written, columns f >= t are not.
 * -1e30f is finite, so no later kernel forms inf - inf, and far below any logit, so an argmax and a softmax ignore those classes.
 * precision 1: h is rounded to bf16 in the kernel, the products accumulate in f32 on the matrix cores (v_mfma_f32_16x16x32_bf16, k
 * ascending), the bias is added in f32.  precision 0: f32 operands on v_mfma_f32_16x16x4_f32 -- the path for tight checks, not a fast one.
 * A workgroup takes 16 frames of ONE clip and up to 256 classes; the frames lie along the lanes of a result tile, so a class row is stored
 * 64 bytes at a time.
 * TS_EINVAL: a NULL pointer (the stream excepted); batch, t, c, n_slots or v_pad <= 0; ldt < t.  TS_EUNSUPPORTED: c % 32 != 0;
 * v_pad % 16 != 0 or v_pad > 4096; batch > 65535; precision not 0 or 1; h, w_bank, bias_bank or logits not 16-byte aligned, vocab or ids not
 * 4-byte aligned; ldt % 4 != 0. */
int ts_mms_lang_bank_head_fwd(const float* h, int32_t batch, int32_t t, int32_t c, const void* w_bank, const float* bias_bank, const int32_t* vocab,
                              int32_t n_slots, int32_t v_pad, const int32_t* ids, float* logits, int32_t ldt, int32_t precision, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* THUNDER_SPEECH_AMD_MMS_LANG_BANK_H */
