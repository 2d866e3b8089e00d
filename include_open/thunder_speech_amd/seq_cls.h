/*
 * thunder_speech_amd/seq_cls.h -- companion C ABI of thunder_speech_amd.h: audio classification heads on the encoders' output
 * (csrc/seq_cls.hip).  transformers' `...ForSequenceClassification` over the wav2vec2 family (the MMS language-identification checkpoints, the
 * SUPERB keyword / intent / emotion checkpoints) is a mean over the valid frames, a projector and a classifier.  All three are linear, so the
 * pool runs first -- a [batch][t][c] tensor shrinks to [batch][c] before any product -- and a weighted sum over the layers' hidden states is
 * the same pool called once per layer with accumulate = 1: a [batch][t][c] layer sum is never formed.
 * The same shared library exports these entry points; the conventions are the core header's (DEVICE pointers into caller-owned buffers,
 * `stream` a hipStream_t passed as void*, 0 / TS_E* / positive hipError_t returns, nothing allocates, frees or synchronises, so every call
 * can be captured into a hipGraph).  It is versioned on its own by TS_SEQ_CLS_ABI_VERSION.
 *
 * No atomics, a fixed summation order: equal arguments give equal bits.  A clip's result depends on nothing outside that clip: a batch gives
 * every clip the bits that clip gives alone.
 *
 * No reference call site: the reference loads CTC checkpoints only (huggingface/compatibility.py:45-112, AutoModelForCTC).
 *
 * Out of scope: fine-tuning classification heads (no backward here); the ...ForAudioFrameClassification and ...ForXVector heads; sew-d and
 * relative-position conformers (refused as before); a confidence threshold or fallback policy for the router; LM fusion, alignment and
 * long-form transcription under a routed selection; downloading checkpoints.
 */
#ifndef THUNDER_SPEECH_AMD_SEQ_CLS_H
#define THUNDER_SPEECH_AMD_SEQ_CLS_H

#include <stdint.h>

#include "thunder_speech_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS_SEQ_CLS_ABI_VERSION 1

/* Version of this companion ABI (a binder checks it next to ts_abi_version). */
int ts_seq_cls_abi_version(void);

/* HOST only: how ts_seq_cls_pool splits the frames of a clip over workgroups.  splits workgroups per clip take rows_per_split consecutive
 * frames each (the last one fewer), block threads each hold 4 consecutive channels.  The split depends on t and c only, never on batch, so a
 * clip alone and the same clip in a batch are summed in the same order.  Any of the three HOST pointers may be NULL.
 * TS_EINVAL: t or c <= 0.  TS_EUNSUPPORTED: c % 8 != 0 or c > 4096. */
int ts_seq_cls_pool_launch_config(int32_t t, int32_t c, int32_t* splits, int32_t* rows_per_split, int32_t* block);

/* Bytes of the partials ts_seq_cls_pool writes and ts_seq_cls_head reads: f32 [batch][splits][c].  0 for arguments either would refuse. */
int64_t ts_seq_cls_pool_workspace_bytes(int32_t batch, int32_t t, int32_t c);

/* The masked mean over time of the encoder's time-major f32 result, as per-split partial sums:
 *   partials[b][s][j]  (+)=  w (1 / len_b) sum_{f in split s, f < len_b} h[b][f][j]         so that
 *   pooled[b][j] = sum_s partials[b][s][j] = w (1 / len_b) sum_{f < len_b} h[b][f][j]        (formed by ts_seq_cls_head, s ascending)
 *   h f32 [batch][t][c];  len int32 [batch] on the device, clamped to [0, t]; NULL: every clip has t frames;
 *   w: ONE f32 read from the device at run time (a captured graph follows a changed layer weight), NULL: 1;
 *   accumulate = 0 sets the partials, accumulate = 1 adds to what an earlier call of the same batch, t and c left there.
 * A clip with len_b = 0 pools to zeros (transformers divides by zero there and returns NaN; that case is not compared with it).
 * One workgroup per (split, clip); a thread sums its 4 channels over the split's frames in frame order.
 * TS_EINVAL: NULL h or partials; batch, t or c <= 0; accumulate not 0 or 1.  TS_EUNSUPPORTED: c % 8 != 0; c > 4096; batch > 65535 (a grid
 * dimension); h or partials not 16-byte aligned; len or w not 4-byte aligned. */
int ts_seq_cls_pool(const float* h, int32_t batch, int32_t t, int32_t c, const int32_t* len, const float* w, int32_t accumulate, float* partials,
                    void* stream);

/* Bytes of ts_seq_cls_head's workspace (the projected vectors z, f32 [batch][p]).  0 for arguments it would refuse. */
int64_t ts_seq_cls_head_workspace_bytes(int32_t batch, int32_t p);

/* The head on the partials ts_seq_cls_pool left for the same batch, t and c (three launches):
 *   pooled[b][j] = sum_s partials[b][s][j], s ascending
 *   z[b][i]      = proj_b[i] + sum_j proj_w[i][j] pooled[b][j]            proj_w [p][c], proj_b f32 [p]
 *   logits[b][l] = cls_b[l] + sum_i cls_w[l][i] z[b][i]                   cls_w [n_labels][p], cls_b f32 [n_labels];  logits f32 [batch][n_labels]
 *   top1[b]      = argmax_l logits[b][l], the lowest index on ties (as ts_greedy_decode)                     int32 [batch], may be NULL
 *   top1_logp[b] = logits[b][top1] - m - log(sum_l exp(logits[b][l] - m)), m the maximum; the maximum and the sum are formed in f32 in class
 *                  order                                                                                      f32 [batch], may be NULL
 *   slot[b]      = class_slot[v], v the argmax over the classes with class_slot[v] >= 0 (lowest index on ties), or -1 when no class is allowed
 *                  class_slot int32 [n_labels] on the device, read at run time; slot int32 [batch]; both NULL, or both given.
 * -1 is what the language bank's launches (thunder_speech_amd/mms_lang_bank.h) read as "the resident language": slot may point into a bank's id
 * buffer.  precision 0: proj_w and cls_w are f32.  precision 1: they are bf16, widened exactly; pooled and z stay f32 and every sum
 * accumulates in f32.  A workgroup holds 32 rows of a weight and up to 4 clips, so a weight is read once per 4 clips; every clip has its own
 * accumulators and a lane's sum runs over its columns in ascending order, then over the 64 lanes in a fixed butterfly.
 * workspace: ts_seq_cls_head_workspace_bytes(batch, p) bytes.
 * TS_EINVAL: NULL partials, proj_w, proj_b, cls_w, cls_b, workspace or logits; batch, t, c, p or n_labels <= 0; class_slot without slot or
 * slot without class_slot.  TS_EUNSUPPORTED: c % 8 != 0 or c > 4096; p % 16 != 0 or p > 4096; n_labels > 8192; batch > 65535; precision not
 * 0 or 1; partials, proj_w, cls_w or workspace not 16-byte aligned; any other pointer not 4-byte aligned. */
int ts_seq_cls_head(const float* partials, int32_t batch, int32_t t, int32_t c, const void* proj_w, const float* proj_b, int32_t p, const void* cls_w,
                    const float* cls_b, int32_t n_labels, const int32_t* class_slot, void* workspace, float* logits, int32_t* top1, float* top1_logp,
                    int32_t* slot, int32_t precision, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* THUNDER_SPEECH_AMD_SEQ_CLS_H */
