/*
 * thunder_speech_amd/queued/lora_bank.h -- queued companion C ABI of thunder_speech_amd.h: a bank of LoRA adaptations served on one frozen base
 * (csrc/lora_bank.hip).  Every clip of a batch picks, by a slot id read on the device at run time, the low-rank pair (A, B) whose term is added
 * to its rows behind the base product: one packed base, many adaptations, one captured graph whatever the mix of adaptations in the batch.  The same
 * shared library exports these entry points; the conventions are the core header's (DEVICE pointers into caller-owned buffers, `stream` a
 * hipStream_t passed as void*, 0 / TS_E* / positive hipError_t returns, nothing allocates, frees or synchronises, so every call can be captured
 * into a hipGraph).  It is versioned on its own by TS_LORA_BANK_ABI_VERSION.
 *
 * QUEUED: this header lives in include_staged/thunder_speech_amd/queued/, one level below the staged companions, because the set of headers in
 * include/ is pinned by tests/test_abi_headers_host.py and the set in include_staged/thunder_speech_amd/ by tests/test_mxfp8_host.py.  The binder
 * reads this directory into a table of its own (_lib.QUEUED) with the same parser.  A later change that edits the pinned tests moves this file
 * into include/thunder_speech_amd/ unchanged.
 *
 * No reference call site: the reference fine-tunes every weight or the CTC head only.  The arithmetic is LoRA's (Hu et al., 2021) as
 * thunder_speech_amd/lora_train.h trains it, so a served adaptation computes what it was trained with.
 *
 * Out of scope: the bank under precision="mxfp8" (it needs the LayerNorm's f32 copy next to the MX operand); banks on the conformer, SEW and
 * MMS-adapter plans; adaptations of different rank in one bank; folding the term into the GEMM epilogue; training with a bank.
 */
#ifndef THUNDER_SPEECH_AMD_QUEUED_LORA_BANK_H
#define THUNDER_SPEECH_AMD_QUEUED_LORA_BANK_H

#include <stdint.h>

#include "thunder_speech_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS_LORA_BANK_ABI_VERSION 1

/* Version of this companion ABI (a binder checks it next to ts_abi_version). */
int ts_lora_bank_abi_version(void);

/* The low-rank terms of up to three target projections that share their input, ONE launch, each clip with the pair of its own slot.
 * Rows of clip b are [b t, (b + 1) t) of x ([batch t][k], row pitch ldx in elements) and of y (row pitch ldy in elements).
 *   a_bank [n_slots][n_targets][r][k], b_bank [n_slots][n_targets][n][r]: bf16 when x_bf16 != 0, else f32 (as x)
 *   scales f32 [n_slots]: alpha / r of the adaptation in the slot (adaptations with different alpha share a bank)
 *   ids    int32 [batch] on the device: clip b uses slot ids[b]
 * Target j adds into columns [col_j, col_j + n) of y; offsets of targets >= n_targets are ignored (pass -1).  x is read once for all targets:
 * u = x [A_0; A_1; A_2]^T is one product.
 *   x_bf16 != 0:  u16 = bf16(x A_j^T) (f32 accumulation on the matrix cores), delta = scales[id] (u16 B_j^T) in f32;
 *                 y_bf16 == 0: f32 y[row][col_j + i] += delta;  y_bf16 != 0: bf16 y = bf16_rne(float(y) + delta)
 *   x_bf16 == 0:  f32 operands, u kept in f32, y f32 (the vector ALUs; precision="fp32" and tight checks, not a fast path)
 * A clip whose id is < 0 or >= n_slots is left untouched: its rows of y keep their bits and nothing of the banks is read for it (-1 selects the
 * base alone; a stale id cannot cause a read outside the banks).  The id is read at run time: a replayed graph serves what ids holds at replay.
 * One workgroup row per clip: a row's result depends on nothing outside its clip; no atomics, a fixed summation order: equal arguments give equal bits.
 * TS_EINVAL: a NULL pointer (the stream excepted); batch, t, k, n, r or n_slots <= 0; n_targets outside 1 .. 3; a used col_j < 0; ldx < k;
 * ldy < col_j + n.  TS_EUNSUPPORTED: r not 8, 16, 32 or 64; k or n not a multiple of 32; batch > 65535; y_bf16 != 0 with x_bf16 == 0;
 * overlapping target column ranges; alignment: x, a_bank, b_bank and y 16-byte aligned, scales and ids 4-byte aligned, ldx a multiple of 8,
 * ldy and every used col_j a multiple of 8 (y_bf16 != 0) or 4 (f32 y), so that every row and slice starts on a 16-byte boundary. */
int ts_lora_bank_fwd(const void* x, int32_t x_bf16, int64_t ldx, int32_t batch, int32_t t, int32_t k,
                     const void* a_bank, const void* b_bank, const float* scales, int32_t n_slots,
                     int32_t n_targets, int32_t n, int32_t r, const int32_t* ids,
                     void* y, int32_t y_bf16, int64_t ldy, int32_t col0, int32_t col1, int32_t col2, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* THUNDER_SPEECH_AMD_QUEUED_LORA_BANK_H */
