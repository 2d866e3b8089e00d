/*
 * thunder_speech_amd/mxfp8.h -- staged companion C ABI of thunder_speech_amd.h: the MXFP8 inference mode of the wav2vec2 encoder layers
 * (precision="mxfp8": OCP e4m3fn elements with one e8m0 scale byte per 32 consecutive K elements, f32 accumulation on the block-scaled
 * matrix-core instruction v_mfma_scale_f32_16x16x128_f8f6f4 of gfx950).  The same shared library exports these entry points; the conventions are
 * the core header's (DEVICE pointers into caller-owned buffers, `stream` a hipStream_t passed as void*, 0 / TS_E* / positive hipError_t returns,
 * nothing allocates, frees or synchronises, so every call can be captured into a hipGraph).  It is versioned on its own by TS_MXFP8_ABI_VERSION.
 *
 * STAGED: this header lives in include_staged/thunder_speech_amd/, next to and not inside include/thunder_speech_amd/, because the set of headers in
 * include/ is pinned by tests/test_abi_headers_host.py.  The binder reads this directory into its own table (_lib.STAGED) with the same parser.  A later
 * change that edits the pinned test moves this file into include/thunder_speech_amd/ unchanged.
 *
 * The quantiser, the same in every entry point that writes an MX operand.  For a block of 32 finite values v (scaled in f32), amax = max|v|:
 *   e = floor(log2(amax)) - 8, plus 1 if amax 2^-e > 448 (the smallest exponent at which nothing saturates), clamped to [-127, 127];
 *   scale byte = e + 127; element = v 2^-e rounded to nearest-even to e4m3fn (subnormals kept, never NaN).  amax == 0: scale byte 0, elements 0x00.
 * The exponent and the comparison are taken from the bits of amax.  Non-finite inputs are out of scope.
 *
 * An "MX operand" below is the pair (elements uint8 [rows][k] with pitch ldq bytes, scales uint8 [rows][k / 32] with pitch lds bytes).
 */
#ifndef THUNDER_SPEECH_AMD_MXFP8_H
#define THUNDER_SPEECH_AMD_MXFP8_H

#include <stdint.h>

#include "thunder_speech_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS_MXFP8_ABI_VERSION 1

/* the output tile of one workgroup of ts_mx_gemm_nt */
#define TS_MX_GEMM_TILE_ROWS 128
#define TS_MX_GEMM_TILE_COLS 128

/* epilogues of ts_mx_gemm_nt */
#define TS_MX_EP_BF16 0      /* y_bf16 = acc + bias                                          (q / k / v)                     */
#define TS_MX_EP_ACCUM 1     /* y += acc (+ bias) in place on the f32 residual stream         (out_proj, second FFN linear)   */
#define TS_MX_EP_GELU_MX 2   /* v = gelu(acc + bias): the MX operand of v, and v in f32 on request   (first FFN linear)      */

/* Version of this companion ABI (a binder checks it next to ts_abi_version). */
int ts_mxfp8_abi_version(void);

/* src [rows][k] (bf16 when src_bf16 != 0, else f32; pitch ld_src elements) -> its MX operand.
 * TS_EINVAL: NULL src / q / scales, rows or k <= 0, a pitch below the row.  TS_EUNSUPPORTED: k % 32 != 0, ld_src % 8 != 0 (bf16) or % 4 != 0 (f32),
 * ldq % 8 != 0, src not 16-byte or q not 8-byte aligned. */
int ts_mx_quantize_rows(const void* src, int32_t src_bf16, int64_t ld_src, int64_t rows, int32_t k, void* q, int64_t ldq, void* scales, int64_t lds,
                        void* stream);

/* The row LayerNorm of ts_w2v_layernorm_fwd without activation, v = LN(x (+ xbias) (+ res)) w + b over rows of c f32 (dense), written as the MX
 * operand of v and, when y is given, as f32 [rows][c]: the MX operand is the quantiser applied to exactly the stored f32 values.
 * TS_EINVAL: NULL x / w / b / q / scales, rows or c <= 0, ldq < c, lds < c / 32.  TS_EUNSUPPORTED: c % 32 != 0 or c > 4096, ldq % 4 != 0, a float
 * pointer not 16-byte or q not 4-byte aligned. */
int ts_mx_layernorm_fwd(const float* x, const float* res, const float* xbias, const float* w, const float* b, float eps, int64_t rows, int32_t c,
                        float* y, void* q, int64_t ldq, void* scales, int64_t lds, void* stream);

/* Bytes of the scale image ts_mx_pack_w writes for a weight [n][k] (the element image has n k bytes); 0 for shapes it does not take. */
int64_t ts_mx_pack_w_scale_bytes(int32_t n, int32_t k);

/* The MX operand of a weight W [n][k], as ts_mx_quantize_rows wrote it, permuted into the fragment order ts_mx_gemm_nt loads: a permutation
 * only, so the product's operand values are exactly the quantiser's.
 *   w_frag [n / 16][k / 128][2][64 lanes][16 bytes]: lane l of half h holds elements [16 nb + (l & 15)][128 s + 64 h + 16 (l >> 4) .. + 15];
 *   s_frag [ceil(n / 64)][k / 128][64 lanes][4 bytes]: byte j of lane l is the scale of row 16 (4 g + j) + (l & 15), block 4 s + (l >> 4)
 *          (row blocks beyond n repeat the last one).
 * TS_EINVAL: a NULL pointer, n or k <= 0, a pitch below the row.  TS_EUNSUPPORTED: n % 16 != 0, k % 128 != 0, ldq % 16 != 0, wq or w_frag not
 * 16-byte or s_frag not 4-byte aligned. */
int ts_mx_pack_w(const void* wq, int64_t ldq, const void* ws, int64_t lds, int32_t n, int32_t k, void* w_frag, void* s_frag, void* stream);

/* acc[m][j] = sum_k x[m][k] w[j][k] over MX operands (x as rows, w packed by ts_mx_pack_w), f32 accumulation; bias f32 [n] or NULL; then by
 * `epilogue`:
 *   TS_MX_EP_BF16     y_bf16 [rows][n] (pitch ld16) = acc + bias
 *   TS_MX_EP_ACCUM    y [rows][n] (f32, pitch ldc) += acc + bias
 *   TS_MX_EP_GELU_MX  v = gelu_erf(acc + bias): (yq, ys) = its MX operand (k of the next product = n); y (optional) = v.  The MX operand is the
 *                     quantiser applied to exactly the f32 values v.
 * Rows beyond `rows` are clamped on the way in and masked on the way out; nothing outside [0, rows) x [0, n) is written.
 * TS_EINVAL: a NULL operand or a NULL output the epilogue needs, rows / n / k <= 0, an epilogue code outside the three, a pitch below its row.
 * TS_EUNSUPPORTED: n % 32 != 0, k % 128 != 0, ldxq % 16 != 0, ldxs % 4 != 0, ldc % 4 != 0, ld16 % 4 != 0, ldyq % 4 != 0, an operand or f32 pointer
 * not 16-byte, y_bf16 not 8-byte, yq or xs not 4-byte aligned, more than 2^31 - 1 tiles, or an operand beyond the kernel's 32-bit offsets:
 * rows ldxq, rows ldxs or n k of 2^31 or more. */
int ts_mx_gemm_nt(const void* xq, int64_t ldxq, const void* xs, int64_t ldxs, const void* w_frag, const void* s_frag, const float* bias,
                  int32_t epilogue, float* y, int64_t ldc, void* y_bf16, int64_t ld16, void* yq, int64_t ldyq, void* ys, int64_t ldys, int64_t rows,
                  int32_t n, int32_t k, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* THUNDER_SPEECH_AMD_MXFP8_H */
