// One layer of data2vec-audio's stacked positional convolutions as a trainable node (include/thunder_speech_amd/posconv_stack_train.h):
//   a = gelu(LN_noaffine(conv(x) + bias)),  LN over the channels with eps 1e-5, no scale / shift (Data2VecAudioPositionalConvLayer).
//   ts_posconv_stack_conv            z = conv(src) alone on the matrix cores: w2v_posconv_mfma_kernel<true> of csrc/w2v_posconv.hip (raw accumulator
//                                    out); forward and, over the flipped / transposed taps, the data gradient
//   ts_posconv_stack_norm_gelu_fwd   a = gelu_erf(LN(z + bias)): one wave per row, the row in registers, one read of z, one write of a
//   ts_posconv_stack_norm_gelu_bwd   dz and the bias gradient from (z, bias, da) in ONE pass over the rows + a small ordered sum
// (the weight gradient is ts_w2v_posconv_wgrad, unchanged; without 64 channels per group the node multiplies on csrc/gemm_f32.hip).
//
// What the backward needs of the forward: NOTHING is saved.  It reads z (which the node keeps anyway: the conv's output) and recomputes mean and
// rstd with the forward's arithmetic -- one more pair of wave reductions per row against 8 bytes per row of statistics that would have to be
// written, kept and read; both kernels are bound by their [rows][c] traffic (forward 8 B per element, backward 12 B).
//
// The row statistics: mean, then the centred values are centred ONCE MORE by their own mean before the sum of squares.  A row that is constant
// across the channels (variance 0) then gives n = 0 to ~1e-11 instead of the 1e-4 that the rounding of sum / c leaves once it is multiplied by
// rstd = 1 / sqrt(eps) = 316.  For the same reason z + bias is pinned as a rounded value before anything is subtracted from it (psn_rounded).
//
// The bias gradient: every workgroup keeps the column sums of dz over ITS rows in registers (per wave), adds its four waves in a fixed order
// through LDS and writes one partial row part[workgroup][c]; psn_bias_reduce_kernel adds the partial rows in a fixed order with plain stores.
// No atomics anywhere: equal arguments give equal bits.
#include "w2v_rows.hpp"

#include "thunder_speech_amd/posconv_stack_train.h"

namespace ts {

namespace {

constexpr int PSN_MAX_PARTS = 1024;     // partial rows of the bias gradient at most (one per workgroup)
constexpr int PSN_ROWS_WG = 8;          // rows per workgroup below that limit: two per wave.  The pair of launches at 3 992 rows x 1024 (768): 4 rows 25.0 (22.2) us,
                                        // 8 rows 19.7 (17.5) us, 16 rows 21.2 (18.8) us (profiles/hubert_data2vec_finetune.md)

__device__ __forceinline__ float psn_gelu_d(float n) {
  return 0.5f * (1.f + erf_as(n * 0.70710678118654752f)) + n * 0.3989422804014327f * __expf(-0.5f * n * n);
}

// The sum z + bias as four rounded f32 values the compiler cannot look through (an empty asm statement: no instruction).  Under -ffast-math the
// backward kernel was otherwise built with (z - mean) + bias, which rounds differently from channel to channel: on a row of variance 0 that noise of
// ~2e-8 is n = 6e-6 after the multiplication by rstd = 316, and 2e-5 of dz (measured; `#pragma clang fp reassociate(off)` did not change the code).
__device__ __forceinline__ f32x4 psn_rounded(f32x4 x) {
#pragma unroll
  for (int i = 0; i < 4; ++i) { float e = x[i]; asm volatile("" : "+v"(e)); x[i] = e; }
  return x;
}

// v[] = z + bias of one row (zeros past c) -> v[] = n = (v - mean) rstd; returns rstd.  The same statements in both kernels.
template <int NV>
__device__ __forceinline__ float psn_normalise(f32x4 (&v)[NV], int lane, int c, float eps) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) s += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
  const float inv_c = 1.f / (float)c;
  const float mu = wave_sum(s) * inv_c;
  float s2 = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const bool in = 4 * (lane + 64 * j) < c;
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[j][i] = in ? v[j][i] - mu : 0.f; s2 += v[j][i]; }
  }
  const float mu2 = wave_sum(s2) * inv_c;              // what the rounding of mu left
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const bool in = 4 * (lane + 64 * j) < c;
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[j][i] = in ? v[j][i] - mu2 : 0.f; q += v[j][i] * v[j][i]; }
  }
  const float rstd = rsqrtf(wave_sum(q) * inv_c + eps);
#pragma unroll
  for (int j = 0; j < NV; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) v[j][i] *= rstd;
  return rstd;
}

// one wave per row (c <= 256 NV, c % 4 == 0): a = gelu_erf(LN(z + bias))
template <int NV>
__global__ __launch_bounds__(256) void psn_fwd_kernel(const float* __restrict__ z, const float* __restrict__ bias, float* __restrict__ a, long long rows, int c,
                                                      float eps) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  f32x4 v[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int col = 4 * (lane + 64 * j);
    v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (col < c) v[j] = psn_rounded(*reinterpret_cast<const f32x4*>(z + row * c + col) + *reinterpret_cast<const f32x4*>(bias + col));
  }
  psn_normalise<NV>(v, lane, c, eps);
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int col = 4 * (lane + 64 * j);
    if (col < c) *reinterpret_cast<f32x4*>(a + row * c + col) = f32x4{gelu_erf(v[j][0]), gelu_erf(v[j][1]), gelu_erf(v[j][2]), gelu_erf(v[j][3])};
  }
}

// dz = rstd (dn - mean(dn) - n mean(dn n)), dn = da gelu'(n); wave w of workgroup g takes the rows 4 g + w, + 4 gridDim.x, ...; the workgroup's column
// sums of dz go to part[g][c] (grid <= PSN_MAX_PARTS workgroups)
template <int NV>
__global__ __launch_bounds__(256) void psn_bwd_kernel(const float* __restrict__ z, const float* __restrict__ bias, const float* __restrict__ da,
                                                      float* __restrict__ dz, float* __restrict__ part, long long rows, int c, float eps) {
  __shared__ f32x4 sm[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  f32x4 db[NV], bv[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int col = 4 * (lane + 64 * j);
    db[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    bv[j] = col < c ? *reinterpret_cast<const f32x4*>(bias + col) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (long long r = (long long)blockIdx.x * 4 + wave; r < rows; r += (long long)gridDim.x * 4) {
    f32x4 v[NV], g[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int col = 4 * (lane + 64 * j);
      v[j] = g[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (col < c) {
        v[j] = psn_rounded(*reinterpret_cast<const f32x4*>(z + r * c + col) + bv[j]);
        g[j] = *reinterpret_cast<const f32x4*>(da + r * c + col);
      }
    }
    const float rstd = psn_normalise<NV>(v, lane, c, eps);
    float m1 = 0.f, m2 = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        g[j][i] *= psn_gelu_d(v[j][i]);                 // dn (0 past c: da was loaded as 0)
        m1 += g[j][i];
        m2 += g[j][i] * v[j][i];
      }
    const float inv_c = 1.f / (float)c;
    m1 = wave_sum(m1) * inv_c;
    m2 = wave_sum(m2) * inv_c;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int col = 4 * (lane + 64 * j);
      if (col < c) {
        f32x4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = rstd * (g[j][i] - m1 - v[j][i] * m2);
        *reinterpret_cast<f32x4*>(dz + r * c + col) = o;
        db[j] += o;
      }
    }
  }
  // the four waves' sums, added in the order ((0 + 1) + (2 + 3)) by wave 0, one 64-float4 slot of the row at a time
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    if (64 * 4 * j < c) {                               // uniform over the workgroup: whole slots past the row's end are skipped
      sm[wave][lane] = db[j];
      __syncthreads();
      const int col = 4 * (lane + 64 * j);
      if (wave == 0 && col < c) *reinterpret_cast<f32x4*>(part + (size_t)blockIdx.x * c + col) = (sm[0][lane] + sm[1][lane]) + (sm[2][lane] + sm[3][lane]);
      __syncthreads();
    }
  }
}

// dbias[col] = sum_p part[p][col] in a fixed order: 16 row groups x 64 columns per workgroup, group q adds the partial rows q, q + 16, ... in order, then
// thread (0, col) adds the 16 group sums in order and stores
__global__ __launch_bounds__(1024) void psn_bias_reduce_kernel(const float* __restrict__ part, float* __restrict__ dbias, int parts, int c) {
  __shared__ float sm[16][64];
  const int cl = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + cl;
  float s = 0.f;
  if (col < c)
    for (int p = q; p < parts; p += 16) s += part[(size_t)p * c + col];
  sm[q][cl] = s;
  __syncthreads();
  if (q == 0 && col < c) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) t += sm[i][cl];
    dbias[col] = t;
  }
}

inline int psn_parts(long long rows) {
  const long long wgs = (rows + PSN_ROWS_WG - 1) / PSN_ROWS_WG;
  return (int)(wgs < PSN_MAX_PARTS ? wgs : PSN_MAX_PARTS);
}

}  // namespace

}  // namespace ts

using namespace ts;

extern "C" int ts_posconv_stack_train_abi_version(void) { return TS_POSCONV_STACK_TRAIN_ABI_VERSION; }

extern "C" int64_t ts_posconv_stack_conv_workspace(int32_t batch, int32_t t, int32_t c, int32_t kernel) {
  if (batch <= 0 || t <= 0 || c <= 0 || kernel <= 0) return TS_EINVAL;
  return ((int64_t)batch * (t + kernel) + 1) * c * 2;
}

/* out = conv(src) on the matrix cores, raw accumulator; see include/thunder_speech_amd/posconv_stack_train.h */
extern "C" int ts_posconv_stack_conv(const float* src, int32_t batch, int32_t t, int32_t c, const void* w_taps_bf16, int32_t kernel, int32_t groups,
                                     int32_t backward, float* out, void* workspace, void* stream_) {
  if (!src || !w_taps_bf16 || !out || !workspace || batch <= 0 || t <= 0 || c <= 0 || kernel <= 1 || groups <= 0 || c % groups) return TS_EINVAL;
  if (c / groups != 64 || c % 4 || (size_t)(128 + kernel - 1) * 144 > 64 * 1024 || misaligned(workspace) || misaligned(src)) return TS_EUNSUPPORTED;
  TS_STREAM;
  return posconv_raw_conv(stream, src, batch, t, c, w_taps_bf16, kernel, groups, backward ? kernel - 1 - kernel / 2 : kernel / 2, out, workspace);
}

extern "C" int ts_posconv_stack_norm_gelu_fwd(const float* z, const float* bias, float eps, int64_t rows, int32_t c, float* a, void* stream_) {
  if (!z || !bias || !a || rows <= 0 || c <= 0) return TS_EINVAL;
  if (c % 4 || c > 4096 || misaligned(z) || misaligned(bias) || misaligned(a)) return TS_EUNSUPPORTED;
  TS_STREAM;
  const dim3 grid((unsigned)((rows + 3) / 4));
#define TS_PSN(NV_) hipLaunchKernelGGL(psn_fwd_kernel<NV_>, grid, dim3(256), 0, stream, z, bias, a, (long long)rows, c, eps)
  if (c <= 512) TS_PSN(2); else if (c <= 1024) TS_PSN(4); else if (c <= 2048) TS_PSN(8); else TS_PSN(16);
#undef TS_PSN
  return hip_status(hipGetLastError());
}

extern "C" int64_t ts_posconv_stack_norm_gelu_bwd_workspace(int64_t rows, int32_t c) {
  if (rows <= 0 || c <= 0) return TS_EINVAL;
  return (int64_t)psn_parts(rows) * c * sizeof(float);
}

extern "C" int ts_posconv_stack_norm_gelu_bwd(const float* z, const float* bias, const float* da, float eps, int64_t rows, int32_t c, float* dz, float* dbias,
                                              void* workspace, void* stream_) {
  if (!z || !bias || !da || !dz || !dbias || !workspace || rows <= 0 || c <= 0) return TS_EINVAL;
  if (c % 4 || c > 4096 || misaligned(z) || misaligned(bias) || misaligned(da) || misaligned(dz) || misaligned(dbias) || misaligned(workspace))
    return TS_EUNSUPPORTED;
  TS_STREAM;
  const int parts = psn_parts(rows);
  float* const part = static_cast<float*>(workspace);
#define TS_PSN(NV_) hipLaunchKernelGGL(psn_bwd_kernel<NV_>, dim3(parts), dim3(256), 0, stream, z, bias, da, dz, part, (long long)rows, c, eps)
  if (c <= 512) TS_PSN(2); else if (c <= 1024) TS_PSN(4); else if (c <= 2048) TS_PSN(8); else TS_PSN(16);
#undef TS_PSN
  hipLaunchKernelGGL(psn_bias_reduce_kernel, dim3((c + 63) / 64), dim3(1024), 0, stream, part, dbias, parts, c);
  return hip_status(hipGetLastError());
}
