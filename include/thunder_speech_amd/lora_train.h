/*
 * thunder_speech_amd/lora_train.h -- companion C ABI of thunder_speech_amd.h: the low-rank (LoRA) term of a frozen linear projection as a trainable node
 * (csrc/lora_train.hip).  It is what LoRA fine-tuning of the attention projections needs next to the launches of the core header: the base
 * product y = x W^T + b and its data gradient dx = dy W stay the core header's bf16 GEMM (ts_gemm_nt_bf16*), these entry points add the low-rank
 * term on top of them.  The same shared library exports these entry points; the conventions are the core header's (DEVICE pointers into
 * caller-owned buffers, `stream` a hipStream_t passed as void*, 0 / TS_E* / positive hipError_t returns, nothing allocates, frees or
 * synchronises, so every call can be captured into a hipGraph).  The core ABI (TS_ABI_VERSION) and the other companions are unchanged by this
 * header; it is versioned on its own by TS_LORA_ABI_VERSION.
 *
 * No reference call site: the reference fine-tunes every weight or the CTC head only.  The arithmetic is LoRA's (Hu et al., 2021) for one target
 * projection with frozen weight W [n][k], rank r and scale s = alpha / r, in mixed precision (bf16 operands, f32 accumulation and results):
 *   u = x A^T   [rows][r]      y = x W^T + b + s u B^T         A [r][k], B [n][r]: bf16 copies of the f32 masters
 *   g = s dy B  [rows][r]      dx = dy W + g A      dA = g^T x  [r][k]      dB = s dy^T u  [n][r]
 * u and g are rounded to bf16 where they become the operand of the next product.
 */
#ifndef THUNDER_SPEECH_AMD_LORA_TRAIN_H
#define THUNDER_SPEECH_AMD_LORA_TRAIN_H

#include <stdint.h>

#include "thunder_speech_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS_LORA_ABI_VERSION 1

/* Version of this companion ABI (a binder checks it next to ts_abi_version). */
int ts_lora_abi_version(void);

/* Forward of one target, ONE launch: u16 [rows][r] bf16 = x16 a16^T (matrix cores, contraction over k), then
 * y[row][0 .. n) += scale * (u16 b16^T) for every row of the f32 matrix y with row pitch ldy (in floats).  y points at the target's first column:
 * the slice may be a part of the [rows][3 c] q | k | v buffer (ldy = 3 c); columns outside [0, n) are not touched, the value already in the
 * slice (the base product and its bias) is kept: result = base + delta.  x16 [rows][k] bf16 (pitch k), a16 [r][k] bf16, b16 [n][r] bf16.
 * u16 is written for the backward (the node saves it: rows r 2 bytes).
 * TS_EINVAL: a NULL pointer (the stream excepted); rows, k, n or r <= 0; ldy < n.  TS_EUNSUPPORTED: r not 8, 16, 32 or 64; k or n not a
 * multiple of 32; ldy not a multiple of 4; a pointer not 16-byte aligned. */
int ts_lora_fwd(const void* x16, int64_t rows, int32_t k, const void* a16, const void* b16, int32_t n, int32_t r, float scale, float* y,
                int64_t ldy, void* u16, void* stream);

/* Backward of one target, three launches (rows; column blocks x row ranges; the ordered sum of the row ranges), no atomics, a fixed summation
 * order: equal arguments give equal bits.
 *   g = bf16(scale * dy16 b16)      dx[row][0 .. k) += g a16  (f32, pitch k; on top of the base product's dx = dy W)
 *   d_a [r][k] f32 = g^T x16        d_b [n][r] f32 = scale * dy16^T u16                     (both set, not added)
 * dy16: the bf16 copy of dy the base product's dx GEMM reads, [rows][n] with row pitch lddy (in elements; the target's slice of a [rows][3 c]
 * copy); x16, u16: what the forward read and wrote.  The two weights come TRANSPOSED, so that the contraction index of each product is the
 * contiguous one: at16 [k][r] = a16^T, bt16 [r][n] = b16^T (bf16; a few KB, transposed by the caller with the cast).
 * dx may be NULL (the first LoRA node above a frozen stack has no upstream gradient to give): the launch then skips that product, d_a and d_b are
 * bit-equal to those of the call with dx.
 * workspace: ts_lora_bwd_workspace bytes, 16-byte aligned; it holds g (f32, [rows][r]) and the partial sums of the row ranges.
 * TS_EINVAL: a NULL required pointer (everything but dx and the stream); rows, k, n or r <= 0; lddy < n.  TS_EUNSUPPORTED: as the forward, with
 * lddy a multiple of 8.  The _workspace function returns a byte count, or the TS_EINVAL / TS_EUNSUPPORTED (< 0) the call
 * would return for these sizes. */
int64_t ts_lora_bwd_workspace(int64_t rows, int32_t k, int32_t n, int32_t r);
int ts_lora_bwd(const void* dy16, int64_t lddy, const void* x16, const void* u16, int64_t rows, int32_t k, int32_t n, int32_t r, float scale,
                const void* at16, const void* bt16, float* dx, float* d_a, float* d_b, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* THUNDER_SPEECH_AMD_LORA_TRAIN_H */
