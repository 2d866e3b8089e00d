/*
 * thunder_speech_amd/qn_head.h -- companion C ABI of include/thunder_speech_amd.h: the end of a QuartzNet forward pass as ONE launch.  The
 * encoder's last block (a 1x1 convolution with folded BatchNorm and ReLU, 512 -> 1024 channels in the reference models) and the conv1d CTC
 * decoder behind it (1024 -> n_classes) run in csrc/qn_head.hip without the hidden tensor ever reaching memory:
 *
 *   h[b, c, t]      = bf16( relu( b17[c] + sum_k W17[c, k] x[b, k, t] ) ),   0 where len_out is given and t >= len_out[b]
 *   logits[b, v, t] = bd[v] + sum_c Wd[v, c] h[b, c, t]
 *
 * The same shared library exports these entry points; the conventions are the core header's (DEVICE pointers into caller-owned buffers,
 * `stream` a hipStream_t passed as void*, 0 / TS_EINVAL / TS_EUNSUPPORTED / positive hipError_t returns, nothing allocates, frees or
 * synchronises, so every call can be captured into a hipGraph).  The core ABI (TS_ABI_VERSION) and the other companions are unchanged by this
 * header; it is versioned on its own by TS_QN_HEAD_ABI_VERSION.
 *
 * Reference call site: the last QuartznetBlock of the encoder followed by conv1d_decoder (quartznet/blocks.py:231-315, blocks.py:199-216),
 * which ts_tcs_subblock_fwd serves as two launches; those stay, for every geometry this header refuses and for callers of the encoder alone.
 */
#ifndef THUNDER_SPEECH_AMD_QN_HEAD_H
#define THUNDER_SPEECH_AMD_QN_HEAD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TS_QN_HEAD_ABI_VERSION 1

/* Frames of a workgroup's tile: rows of x must be readable up to the end of the last tile. */
#define TS_QN_HEAD_TILE 96
/* Largest n_classes, hidden-channel granule (eight waves x 64 channels) and cap (the shift lives in LDS), largest c_in (the [c_in][96] tile lives
 * in LDS). */
#define TS_QN_HEAD_V_MAX 32
#define TS_QN_HEAD_HIDDEN_STEP 512
#define TS_QN_HEAD_HIDDEN_MAX 4096
#define TS_QN_HEAD_CIN_MAX 512

/* Version of this companion ABI (a binder checks it next to ts_abi_version). */
int ts_qn_head_abi_version(void);

/* Launches ts_qn_head_fwd has made in this process so far (a refused call does not count): lets a caller tell which path served a forward. */
int64_t ts_qn_head_launches(void);

/* One launch for both layers.
 *   x            bf16 [batch][c_in][pitch_in], 16-byte aligned, with the tail-zero invariant (frames >= the clip's length are 0); it is
 *                read unmasked
 *   len_out      int32 [batch] or NULL.  Given: h counts as 0 from frame len_out[b] on (clamped to [0, t_out]), so those frames' logits are
 *                bd.  NULL: no frame is masked (with a tail-zero x the frames beyond a clip's length then carry bd + Wd relu(b17), what the
 *                two separate launches leave there)
 *   w17, b17     the first layer as ts_tcs_subblock_fwd takes it: BN-folded bf16 weight fragments of v_mfma_f32_16x16x32_bf16
 *                [hidden / 16][c_in / 32][64][8] (ts_tcs_desc.pw_w16) and the f32 shift [hidden]
 *   wd           bf16 [hidden / 64][2][2][64][8]: the decoder's weights as A fragments whose k-order follows the first layer's accumulator
 *                layout -- fragment (g, p, vt), lane l, element e holds Wd[16 vt + (l & 15)][64 g + 16 (2 p + (e >> 2)) + 4 (l >> 4) + (e & 3)],
 *                0 for rows >= n_classes
 *   bd           f32 [n_classes]
 *   logits       f32 [batch][n_classes][pitch_out], 4-byte aligned; frames [0, t_out) of every row are written, nothing else
 *   kernel, stride, c_res   the first layer's geometry: 1, 1 and 0 (no residual branch), anything else is refused
 * Arithmetic: h accumulates in f32 from the shift upwards in ascending k, as the split kernel does, and is rounded to bf16 once; each
 * wave's partial logits are f32 sums, joined through LDS in wave order.  No atomics: two calls give the same bits.
 * TS_EINVAL: a NULL pointer (len_out and the stream excepted), batch <= 0, c_in <= 0, hidden <= 0, n_classes <= 0, t_out <= 0.
 * TS_EUNSUPPORTED: n_classes > TS_QN_HEAD_V_MAX, c_in not a multiple of 64 or above TS_QN_HEAD_CIN_MAX, hidden not a multiple of
 * TS_QN_HEAD_HIDDEN_STEP or above TS_QN_HEAD_HIDDEN_MAX, kernel != 1, stride != 1, c_res != 0, pitch_in not a multiple of 8 or below round_up(t_out, TS_QN_HEAD_TILE),
 * pitch_out < t_out, a clip of x (c_in x pitch_in bf16) or the tile count beyond 2^31 - 1, x / w17 / wd / b17 not 16-byte aligned, bd / logits / len_out not 4-byte aligned.  All of these return before any
 * device call. */
int ts_qn_head_fwd(const void* x, const int32_t* len_out, const void* w17, const float* b17, const void* wd, const float* bd, float* logits,
                   int32_t batch, int32_t c_in, int32_t hidden, int32_t n_classes, int32_t t_out, int32_t pitch_in, int32_t pitch_out,
                   int32_t kernel, int32_t stride, int32_t c_res, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* THUNDER_SPEECH_AMD_QN_HEAD_H */
