// The activation-row conventions of the training kernels, one copy for csrc/train_dw.hip, train_bn.hip, train_rows.hip, train_extra.hip,
// train_gemm.hip and w2v_train.hip.  Activations are [B][C][pitch] rows (time contiguous, pitch a multiple of 8 elements, 16-byte aligned rows;
// columns >= T are scratch) in one of two element types, selected per call by `act`: 0 = f32 (the reference's arithmetic), 1 = bf16 storage with
// f32 arithmetic inside every kernel (mixed precision: half the activation traffic, bf16 MFMA GEMMs; parameters, gradients of parameters,
// statistics stay f32).
#pragma once
#include "ts_common.hpp"      // wave_sum, TS_STREAM

namespace ts {

__device__ __forceinline__ int clamp_len(const int* len, int b, int t) {
  if (!len) return t;
  const int l = len[b];
  return l < 0 ? 0 : (l > t ? t : l);
}

// element access of the two activation types (f32 / bf16 bits)
typedef unsigned short bf16_t;
__device__ __forceinline__ float ldf(const float* p, size_t i) { return p[i]; }
__device__ __forceinline__ float ldf(const bf16_t* p, size_t i) { return bf16_to_f32(p[i]); }
__device__ __forceinline__ void stf(float* p, size_t i, float v) { p[i] = v; }
__device__ __forceinline__ void stf(bf16_t* p, size_t i, float v) { p[i] = (bf16_t)(pack_bf16(v, 0.f) & 0xffffu); }
// 8 consecutive elements of a 16-byte aligned row position
__device__ __forceinline__ void load8(const float* p, float (&v)[8]) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
  v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3]; v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
}
__device__ __forceinline__ void load8(const bf16_t* p, float (&v)[8]) {
  const u32x4 a = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
  for (int j = 0; j < 4; ++j) { v[2 * j] = bf16_lo(a[j]); v[2 * j + 1] = bf16_hi(a[j]); }
}
// Activation rows leave with plain stores.  Streaming (nontemporal) stores were built and measured on the training step: +4 % -- a launch writes
// 8-16 MB that the NEXT launch reads, and streaming the lines out evicts what that launch would hit in L2.
__device__ __forceinline__ void st16(u32x4* p, u32x4 v) { *p = v; }
__device__ __forceinline__ void st16(f32x4* p, f32x4 v) { *p = v; }
__device__ __forceinline__ void store8(float* p, const float (&v)[8]) {
  st16(reinterpret_cast<f32x4*>(p), f32x4{v[0], v[1], v[2], v[3]});
  st16(reinterpret_cast<f32x4*>(p + 4), f32x4{v[4], v[5], v[6], v[7]});
}
__device__ __forceinline__ void store8(bf16_t* p, const float (&v)[8]) {
  st16(reinterpret_cast<u32x4*>(p), u32x4{pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]), pack_bf16(v[4], v[5]), pack_bf16(v[6], v[7])});
}

// ----------------------------------------------------------------------------------------------------------------------
// Row-wise streaming kernels: one WAVE = one (row, 512-frame chunk) unit, 64 lanes x 8 elements (16 / 32 bytes per lane), four
// units per 256-thread workgroup (a 10 s clip is 501 frames: with one workgroup per row three of its four waves had nothing to do).
// Rows are pitched and 16-byte aligned, so every access is a whole vector; columns >= t are scratch and may be overwritten.
// ----------------------------------------------------------------------------------------------------------------------
constexpr int ROW_CHUNK = 512;
// defines `row`, `chunk`, `i` (first frame of this lane) and returns from the kernel when the unit lies outside the tensor
#define TS_ROW_UNIT(n_rows)                                                                   \
  const int _cpr = (t + ROW_CHUNK - 1) / ROW_CHUNK;                                           \
  const long long _u = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);                        \
  const long long _r = _u / _cpr;                                                             \
  const int row = (int)_r, chunk = (int)(_u % _cpr), i = chunk * ROW_CHUNK + (threadIdx.x & 63) * 8; \
  if (_r >= (long long)(n_rows) || i >= t) return

static inline unsigned blocks(long long n) { return (unsigned)((n + 255) / 256); }
static inline dim3 row_grid(long long rows, int t) { return dim3((unsigned)((rows * ((t + ROW_CHUNK - 1) / ROW_CHUNK) + 3) / 4)); }
static inline bool rows_ok(const void* p, int pitch, int act) {
  return pitch % 8 == 0 && reinterpret_cast<uintptr_t>(p) % (act ? 16 : 32) == 0;
}

// ---- BatchNorm(train) statistics of one channel ----
constexpr int BN_G = 8;                                   // clip groups of the BatchNorm partial sums
__device__ __forceinline__ void bn_total(const double* __restrict__ part, int ch, int c, double& s1, double& s2, int ng = BN_G) {
  s1 = 0.0; s2 = 0.0;
  for (int g = 0; g < ng; ++g) { s1 += part[((size_t)g * ch + c) * 2]; s2 += part[((size_t)g * ch + c) * 2 + 1]; }
}
// the channel's totals out of the per-tile pairs: the 64 lanes of a wave share the tiles, then combine (every lane of the wave must call this)
__device__ __forceinline__ void bn_total_tiles(const float* __restrict__ tiles, int n_tiles, int ch, int c, int lane, double& s1, double& s2) {
  double a1 = 0.0, a2 = 0.0;
  const float* const row = tiles + (size_t)c * n_tiles * 2;
  for (int p = lane; p < n_tiles; p += 64) { a1 += (double)row[2 * p]; a2 += (double)row[2 * p + 1]; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { a1 += __shfl_xor(a1, o); a2 += __shfl_xor(a2, o); }
  s1 = a1; s2 = a2;
}
// A constant that the compiler folds only AFTER the helper it is handed to has been inlined.  A helper whose every caller in a translation unit
// passes the same constant is specialised on it beforehand (bn_total's loop is then unrolled inside the helper), and the kernels around it get
// another schedule: dw_fwd_pair_kernel had 47 instructions more, all scalar spills, than it has with the group count passed this way.
__device__ __forceinline__ int late_const(int v) { return __builtin_amdgcn_readfirstlane(v); }
// The finalisation that follows the totals (mean, clamped biased variance, rstd, mean_rstd published, running statistics blended) is written out
// at its five sites.  Under -ffast-math their momentum blends (1 - m) r + m x round in two ways -- two products and a sum in bn_fwd_kernel and
// dw_fwd_mfma_kernel, r + m (x - r) in row_affine(PairBnIn), bn2_add_relu_kernel and bn2_fwd_chan_kernel -- so unifying them changes results.

// ---- launch dispatch on the activation type ----
// act_dispatch(act, [&](auto tag) { using T = decltype(tag); ... kernel<T> ... as<T>(ptr) ... }) runs the body with T = float (act 0) or bf16_t (act 1)
template <class F> static inline void act_dispatch(int act, F&& body) { if (act) body(bf16_t{}); else body(float{}); }
template <class T> static inline const T* as(const void* p) { return static_cast<const T*>(p); }
template <class T> static inline T* as(void* p) { return static_cast<T*>(p); }

}  // namespace ts
