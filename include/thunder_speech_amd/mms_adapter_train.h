/*
 * thunder_speech_amd/mms_adapter_train.h -- companion C ABI of thunder_speech_amd.h: the MMS attention adapter as a trainable node, an
 * out-of-place forward and a fused backward (csrc/mms_adapter_train.hip).  It is what adapter-only fine-tuning of an MMS checkpoint needs next
 * to the launches of the core header and of thunder_speech_amd/mms_train.h: the base is frozen, the adapters (and the CTC head) train.  The same
 * shared library exports these entry points; the conventions are the core header's (DEVICE pointers into caller-owned buffers, `stream` a
 * hipStream_t passed as void*, 0 / TS_E* / positive hipError_t returns, nothing allocates, frees or synchronises, so every call can be captured
 * into a hipGraph).  The core ABI (TS_ABI_VERSION) and the other companions are unchanged by this header; it is versioned on its own by
 * TS_MMS_ADAPTER_TRAIN_ABI_VERSION.
 *
 * Reference call site: transformers' Wav2Vec2AttnAdapterLayer at the end of Wav2Vec2EncoderLayerStableLayerNorm.forward under the reference's
 * training_step, after init_adapter_layers() / freeze_base_model() / unfreezing _get_adapters().  Per row of the f32 residual stream h [rows][c]:
 *   u = LN(h; norm_w, norm_b, eps 1e-5),  z = W1 u + b1,  r = relu(z),  y = h + W2 r + b2;   W1 [a][c], W2 [c][a] (nn.Linear layout), b1 [a], b2 [c]
 */
#ifndef THUNDER_SPEECH_AMD_MMS_ADAPTER_TRAIN_H
#define THUNDER_SPEECH_AMD_MMS_ADAPTER_TRAIN_H

#include <stdint.h>

#include "thunder_speech_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS_MMS_ADAPTER_TRAIN_ABI_VERSION 1

/* Version of this companion ABI (a binder checks it next to ts_abi_version). */
int ts_mms_adapter_train_abi_version(void);

/* Forward: y [rows][c] f32 = the adapter applied to h, which is left untouched (autograd keeps it).  The kernel and the arithmetic are those of
 * ts_mms_attn_adapter_fwd (thunder_speech_amd/mms.h) without a fused LayerNorm behind it: for equal inputs and precision, y equals bit for bit
 * what that call leaves in a copy of h.
 * precision 0: w1 / w2 f32, every product on the f32 matrix-core instruction.  precision 1: w1 / w2 bf16, u and r rounded to bf16 for the two
 * products (f32 accumulation); LayerNorm and the sum into y f32.
 * TS_EINVAL: a NULL pointer (the stream excepted); rows, c or a <= 0.  TS_EUNSUPPORTED: a % 16 != 0 or a > 64; c % 8 != 0 or c > 4096; precision
 * not 0 or 1; a pointer not 16-byte aligned. */
int ts_mms_attn_adapter_train_fwd(const float* h, int64_t rows, int32_t c, int32_t a, const float* norm_w, const float* norm_b, const void* w1,
                                  const float* b1, const void* w2, const float* b2, float* y, int32_t precision, void* stream);

/* Backward, from h and dy [rows][c] f32 alone: u, z and the ReLU mask are recomputed (with the forward's arithmetic, so the mask is the forward's);
 * nothing of size [rows][c] is kept by the forward or stored here except dh.
 *   d_b2 [c] = sum_rows dy                 d_w2 [c][a] = sum_rows dy (x) r          dz = (dy W2) . [z > 0]
 *   d_b1 [a] = sum_rows dz                 d_w1 [a][c] = sum_rows dz (x) u          du = dz W1
 *   d_norm_w [c] = sum_rows du . xhat      d_norm_b [c] = sum_rows du               dh [rows][c] = dy + LayerNorm backward of du . norm_w
 * dh may be NULL (the first adapter of a frozen base has no upstream gradient): the launch then skips du's product and the LayerNorm backward, and
 * the six parameter gradients are bit-equal to those of the call with dh.  The six parameter gradients (all f32) are always written over
 * whatever the buffers held: set, not added.
 * precision 0: w1 / w2 f32, products in f32.  precision 1: w1 / w2 bf16; u, r, dy and dz are rounded to bf16 for the products, f32 accumulation;
 * LayerNorm, its backward and every sum over rows (the three bias / scale gradients) stay f32.
 * Three launches (rows; column blocks x row ranges; the ordered sum of the row ranges), no atomics, a fixed summation order: equal arguments give
 * equal bits.  workspace: ts_mms_attn_adapter_train_bwd_workspace bytes, 16-byte aligned; it holds the row statistics, r and dz (width a) and the
 * partial sums of the row ranges -- nothing of width c per row.
 * TS_EINVAL: a NULL required pointer (everything but dh and the stream); rows, c or a <= 0.  TS_EUNSUPPORTED: as the forward.  The _workspace
 * function returns a byte count, or TS_EINVAL (< 0) for a non-positive argument. */
int64_t ts_mms_attn_adapter_train_bwd_workspace(int64_t rows, int32_t c, int32_t a);
int ts_mms_attn_adapter_train_bwd(const float* h, const float* dy, int64_t rows, int32_t c, int32_t a, const float* norm_w, const float* norm_b,
                                  const void* w1, const float* b1, const void* w2, float* dh, float* d_norm_w, float* d_norm_b, float* d_w1,
                                  float* d_b1, float* d_w2, float* d_b2, void* workspace, int32_t precision, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* THUNDER_SPEECH_AMD_MMS_ADAPTER_TRAIN_H */
