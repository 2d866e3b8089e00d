// The row conventions of the wav2vec2-family kernels, one copy for csrc/w2v_conv.hip, w2v_rows.hip, w2v_posconv.hip, w2v_attn.hip, wavlm.hip,
// conformer.hip, w2v_train.hip and the epilogue of csrc/gemm_nt.hip: the erf-GELU / SiLU activations, the key-length clamp and the row softmax
// of the unfused attention paths.  (wave_sum / wave_max and the host side of the launchers -- TS_STREAM, nblk, misaligned, the prototypes of
// the library's GEMMs -- are csrc/ts_common.hpp's.)
// NOT here: the LayerNorm row (NV float4 per lane: load, mean, centred sum of squares, rsqrtf) of w2v_layernorm_kernel, conformer_ln_rotary_kernel
// and ln_bwd_kernel.  Under -ffast-math the compiler picks the association of the four-element sums and the contraction of x - mean per
// kernel; every shared form that was built (array by reference, row by value, one function or two) changed them, i.e. the results
// (profiles/w2v_enc_split.md).  A new kernel copies the row from w2v_layernorm_kernel.
#pragma once
#include "ts_common.hpp"

namespace ts {

// erf by Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7, below fp32 GELU noise; a third of the instructions of ocml's erff: the conv0 and
// epilogue kernels are bound by exactly this)
__device__ __forceinline__ float erf_as(float x) {
  const float ax = fabsf(x);
  const float t = __frcp_rn(fmaf(0.3275911f, ax, 1.f));
  const float poly = t * fmaf(t, fmaf(t, fmaf(t, fmaf(t, 1.061405429f, -1.453152027f), 1.421413741f), -0.284496736f), 0.254829592f);
  const float r = 1.f - poly * __expf(-ax * ax);
  return copysignf(r, x);
}
__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.f + erf_as(x * 0.70710678118654752f)); }
__device__ __forceinline__ float silu(float x) { return x / (1.f + __expf(-x)); }
// The same erf written with a division and a compare, as gelu_kernel, ffn_act_cast_kernel and ffn_act_bwd_kernel (csrc/w2v_train.hip) were built
// with: the same float operations, but the sign comes from v_cmp + v_cndmask instead of v_bfi (it differs from erf_as at -0 and NaN only, where
// neither GELU nor its derivative can tell), and with erf_as those three kernels are scheduled differently.  Kept so that they compile to the
// code they were measured with; new kernels take erf_as.
__device__ __forceinline__ float erf_as_div(float x) {
  const float ax = fabsf(x);
  const float t = 1.f / (1.f + 0.3275911f * ax);
  const float y = 1.f - (((((1.061405429f * t - 1.453152027f) * t) + 1.421413741f) * t - 0.284496736f) * t + 0.254829592f) * t * __expf(-ax * ax);
  return x < 0.f ? -y : y;
}

// ---- attention rows ----
// len[b] clamped to [0, t]: the number of valid keys (rows) of clip b.  What an EMPTY clip (0) means is the caller's: the inference kernels then
// attend to all t keys (the reference's softmax over equally masked keys); the fused kernels take csrc/attn_tile.hpp's key_limit<ALL_IF_EMPTY>
__device__ __forceinline__ int key_limit(const int* len, int b, int t) { return len[b] < t ? (len[b] < 0 ? 0 : len[b]) : t; }

// Softmax of one row of scores by one wave over the keys [0, lim): probability exp(s[i] scale - m) / sum; the keys lim .. end - 1 get 0.
// softmax_row_max gives m; softmax_row_finish does the rest and hands (i, probability) to `store` (which may overwrite s[i]; a lambda that
// captures its pointers BY VALUE -- through a by-reference capture w2v_softmax_kernel lost the per-lane form of its bf16 / f32 branch).
__device__ __forceinline__ float softmax_row_max(const float* s, int lim, float scale, int lane) {
  float m = -3.0e38f;
  for (int i = lane; i < lim; i += 64) m = fmaxf(m, s[i] * scale);
  return wave_max(m);
}
template <class Store>
__device__ __forceinline__ void softmax_row_finish(const float* s, int lim, int end, float scale, float m, int lane, Store store) {
  float z = 0.f;
  for (int i = lane; i < lim; i += 64) z += __expf(s[i] * scale - m);
  const float rz = 1.f / wave_sum(z);
  for (int i = lane; i < end; i += 64) store(i, i < lim ? __expf(s[i] * scale - m) * rz : 0.f);
}

}  // namespace ts
