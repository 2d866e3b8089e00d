// SEW (transformers' SEWModel, the squeezed wav2vec2): the two launches its encoder needs next to the wav2vec2 ones, time-major fp32 [B][T][C];
// ABI in include/thunder_speech_amd/sew.h.
//   ts_sew_squeeze_fwd      y[r] = mean_{i < s} x[s r + i] + gelu(conv_stride_s(x)[r] + b), T / s output frames: precision 1 with 24 or 32 channels per
//                           group on sew_squeeze_mfma_kernel; otherwise the f32 GEMM (csrc/gemm_f32.hip, one launch: the taps are its outer
//                           contraction loop, the stride its row pitch) over a padded f32 copy and sew_squeeze_finish_kernel
//   ts_sew_unsqueeze_rows   the upsampler's [B][T2][s C] rows as [B][T][C] with zero rows behind s T2 (only when T % s != 0)
#include <type_traits>

#include "w2v_rows.hpp"

#include "thunder_speech_amd/sew.h"
#include "sew_squeeze.hpp"

namespace ts {

// ---------------------------------------------------------------------------------------------------------------------
// The strided positional conv as an implicit GEMM on the matrix cores (precision 1; 32 channels per group, or 24 packed as 32).
//   workgroup = 128 output frames x TWO groups of one clip; the 127 s + k input rows it needs are staged ONCE in LDS as bf16, 64 channels wide
//   (two 32-channel slots), and tap j reads window rows s f + j.  The window is stored split by phase -- row r at slot (r % s) rpp + r / s -- so
//   the 32 frames of an A fragment, s rows apart in the clip, are CONSECUTIVE slots: the ds_read_b128 pattern is the one of w2v_posconv_mfma_kernel
//   (pitch 144 B: the 16 lanes of a read group fall on 16 different 16-byte bank groups), where rows at pitch 2 x 144 B would be 2-way conflicts
//   for every 16-byte-aligned pitch.
//   waves 2 x 2: 64 frames x the 32 output channels of one group each, v_mfma_f32_32x32x16_bf16, two k-steps per tap; B = tap weights [co][ci]
//   straight from L2, prefetched a block of four taps ahead.  Epilogue: + bias, GELU, + the average pool of the fp32 x, coalesced along channels.
// With 24 channels per group the padded copy and the packed weights carry zeros in channels 24 .. 31 of each slot: the same kernel.
// ---------------------------------------------------------------------------------------------------------------------
// (SQ_TT output frames per workgroup, SQ_PITCH bytes per staged row, SQ_SLOT channels per group in the padded copy and the packed weights, SQ_LDS_MAX:
// csrc/sew_squeeze.hpp, shared with the training launches of csrc/sew_train.hip)
constexpr int SQ_TB = 4;           // taps per block of prefetched weights
constexpr int SQ_SB = 6;           // staging loads in flight per thread

struct SqArgs {
  const unsigned short* xp;        // [B][prow][groups x 32] bf16, k / 2 zero rows in front of each clip
  const unsigned short* w;         // [k][groups][32 co][32 ci] bf16
  const float* bias;
  const float* x;                  // [B][T][C] fp32 (average pool)
  float* y;                        // [B][T2][C]
  float* z;                        // SAVE_Z (ts_sew_squeeze_train_fwd): [B][T2][C], the conv result before bias and GELU
  int t, t2, c, cg, cp, k, groups, stride, prow, rpp;       // cp = groups x 32; rpp = window slots per phase
};

// SAVE_Z: the training forward, which also stores the accumulator as it is; <false> is the inference kernel as it was.
template <bool SAVE_Z>
__global__ __launch_bounds__(256) void sew_squeeze_mfma_kernel(const SqArgs a) {
  extern __shared__ __attribute__((aligned(16))) char win[];                  // [stride][rpp][SQ_PITCH]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, gp = blockIdx.y, r0 = blockIdx.x * SQ_TT;
  const int rows = (SQ_TT - 1) * a.stride + a.k;
  const long long row0 = (long long)r0 * a.stride;                           // the window's first row in the clip's padded copy
  const unsigned short* src = a.xp + ((size_t)b * a.prow + row0) * a.cp + (size_t)gp * 64;
  // 16-byte chunks, SQ_SB per thread in flight at a time (one load per round trip would leave the window's twelve rounds as twelve memory latencies)
  for (int base = tid; base < rows * 8; base += 256 * SQ_SB) {
    uint4 v[SQ_SB];
#pragma unroll
    for (int u = 0; u < SQ_SB; ++u) {
      const int chunk = base + 256 * u, r = chunk >> 3, cc = chunk & 7;
      v[u] = uint4{0u, 0u, 0u, 0u};
      if (chunk < rows * 8 && row0 + r < a.prow && gp * 64 + cc * 8 < a.cp)                                  // an odd group count: no second slot
        v[u] = *reinterpret_cast<const uint4*>(src + (size_t)r * a.cp + cc * 8);
    }
#pragma unroll
    for (int u = 0; u < SQ_SB; ++u) {
      const int chunk = base + 256 * u, r = chunk >> 3, cc = chunk & 7;
      const int q = r / a.stride, p = r - q * a.stride;
      if (chunk < rows * 8) *reinterpret_cast<uint4*>(win + (p * a.rpp + q) * SQ_PITCH + cc * 16) = v[u];
    }
  }
  __syncthreads();
  const int wm = wave >> 1, wn = wave & 1;                                    // 64 frames x one group's 32 channels per wave
  const int g = gp * 2 + wn;
  if (g >= a.groups) return;                                                  // no barrier follows
  const int half = lane >> 5, n32 = lane & 31;
  f32x16 acc[2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[mt][i] = 0.f;
  const char* arow = win + (wm * 64 + n32) * SQ_PITCH + wn * 64 + half * 16;  // A: row = frame, 8 consecutive ci per k-step
  const uint4* wp = reinterpret_cast<const uint4*>(a.w + ((size_t)g * SQ_SLOT + n32) * SQ_SLOT + 8 * half);
  const size_t tap_stride = (size_t)a.groups * SQ_SLOT * SQ_SLOT / 8;         // uint4 units
  // Tap weights travel in blocks of SQ_TB taps through two register sets: while one block is multiplied (SQ_TB x 4 MFMAs) the next one's loads are
  // in flight, and the wait in front of a block leaves the younger block's loads outstanding.  (One tap ahead in rotating registers, the wait before
  // each tap's first MFMA also covered the load just issued: an L2 round trip per tap.)  Loads past the last tap re-read it; nothing is multiplied by them.
  uint4 b0[SQ_TB][2], b1[SQ_TB][2];
  auto load_taps = [&](uint4 (&bw)[SQ_TB][2], int j0) {
#pragma unroll
    for (int u = 0; u < SQ_TB; ++u) {
      const int j = j0 + u < a.k ? j0 + u : a.k - 1;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) bw[u][ks] = wp[(size_t)j * tap_stride + 2 * ks];
    }
  };
  int p = 0, q = 0;                                                           // tap j = q stride + p
  auto run_taps = [&](const uint4 (&bw)[SQ_TB][2], int j0, auto guarded) {     // guarded: the block may reach past the last tap
#pragma unroll
    for (int u = 0; u < SQ_TB; ++u) {
      if (!decltype(guarded)::value || j0 + u < a.k) {
        const char* at = arow + (p * a.rpp + q) * SQ_PITCH;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int mt = 0; mt < 2; ++mt) {
            const s16x8 af = *reinterpret_cast<const s16x8*>(at + 32 * mt * SQ_PITCH + ks * 32);
            acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, __builtin_bit_cast(s16x8, bw[u][ks]), acc[mt], 0, 0, 0);
          }
        if (++p == a.stride) { p = 0; ++q; }
      }
    }
  };
  load_taps(b0, 0);
  int j0 = 0;
  for (; j0 + 2 * SQ_TB <= a.k; j0 += 2 * SQ_TB) {                            // whole blocks: straight-line code, the LDS reads of a block are free to move up
    load_taps(b1, j0 + SQ_TB);
    run_taps(b0, j0, std::false_type{});
    load_taps(b0, j0 + 2 * SQ_TB);
    run_taps(b1, j0 + SQ_TB, std::false_type{});
  }
  if (j0 < a.k) {
    load_taps(b1, j0 + SQ_TB);
    run_taps(b0, j0, std::true_type{});
    run_taps(b1, j0 + SQ_TB, std::true_type{});
  }
  if (n32 >= a.cg) return;                                                    // the zero channels of a 24-channel group
  const int co = g * a.cg + n32;
  const float bv = a.bias[co], inv = 1.f / (float)a.stride;
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int f = r0 + wm * 64 + 32 * mt + 8 * (i >> 2) + 4 * half + (i & 3);
      if (f < a.t2) {
        const float* xr = a.x + ((size_t)b * a.t + (size_t)f * a.stride) * a.c + co;
        float pool = xr[0];
        for (int s = 1; s < a.stride; ++s) pool += xr[(size_t)s * a.c];
        if constexpr (SAVE_Z) a.z[((size_t)b * a.t2 + f) * a.c + co] = acc[mt][i];
        a.y[((size_t)b * a.t2 + f) * a.c + co] = pool * inv + gelu_erf(acc[mt][i] + bv);
      }
    }
}

// bf16 copy of x [B][t][groups x cg] f32 as [B][prow][groups x 32]: `front` zero rows before each clip, zeros behind it and in channels cg .. 31 of
// each slot; four elements per thread (cg % 4 == 0)
__global__ __launch_bounds__(256) void sew_pad16_kernel(const float* __restrict__ x, unsigned short* __restrict__ xp, int t, int c, int cg, int cp, int prow,
                                                        int front, long long total) {
  const long long idx = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (idx >= total) return;
  const long long row = idx / cp;
  const int col = (int)(idx - row * cp);
  const long long b = row / prow;
  const int r = (int)(row - b * prow) - front;
  const int g = col / SQ_SLOT, ci = col - g * SQ_SLOT;
  f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
  if (r >= 0 && r < t && ci < cg) v = *reinterpret_cast<const f32x4*>(x + ((size_t)b * t + r) * c + g * cg + ci);
  *reinterpret_cast<u32x2*>(xp + idx) = u32x2{pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3])};
}

// ---------------------------------------------------------------------------------------------------------------------
// f32 path: padded f32 copy [B][prow][C] (prow a multiple of the stride, so that output frame r of clip b is row b prow / s + r of ONE strided
// row space), the conv on gemm_f32, then pool + bias + GELU
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sew_pad32_kernel(const float* __restrict__ x, float* __restrict__ xp, int t, int c, int prow, int front) {
  const int b = blockIdx.y;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = (long long)prow * c;
  if (idx >= total) return;
  const long long r = idx / c;
  const int col = (int)(idx - r * c);
  const long long src = r - front;
  xp[(size_t)b * total + idx] = (src >= 0 && src < t) ? x[((size_t)b * t + src) * c + col] : 0.f;
}

__global__ __launch_bounds__(256) void sew_squeeze_finish_kernel(const float* __restrict__ x, const float* __restrict__ yp, const float* __restrict__ bias,
                                                                 float* __restrict__ y, int t, int t2, int c, int stride, long long clip_rows) {
  const int b = blockIdx.y;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)t2 * c) return;
  const long long r = idx / c;
  const int col = (int)(idx - r * c);
  const float* xr = x + ((size_t)b * t + (size_t)r * stride) * c + col;
  float pool = xr[0];
  for (int s = 1; s < stride; ++s) pool += xr[(size_t)s * c];
  const float v = yp[((size_t)b * clip_rows + r) * c + col] + bias[col];
  y[(size_t)b * t2 * c + idx] = pool * (1.f / (float)stride) + gelu_erf(v);
}

// dst [B][t][c] = the n_src floats of each clip of src, then zeros: 16 bytes per thread
__global__ __launch_bounds__(256) void sew_unsqueeze_rows_kernel(const float* __restrict__ src, float* __restrict__ dst, long long n_src, long long n_dst) {
  const int b = blockIdx.y;
  const long long idx = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (idx >= n_dst) return;
  f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
  if (idx < n_src) v = *reinterpret_cast<const f32x4*>(src + (size_t)b * n_src + idx);
  *reinterpret_cast<f32x4*>(dst + (size_t)b * n_dst + idx) = v;
}

}  // namespace ts

using namespace ts;

void ts::sew_pad16(hipStream_t stream, const float* x, unsigned short* xp, int batch, int t, int c, int groups, long long prow, int front) {
  const int cp = groups * SQ_SLOT;
  const long long total = (long long)batch * prow * cp;
  hipLaunchKernelGGL(sew_pad16_kernel, dim3(nblk(total / 4)), dim3(256), 0, stream, x, xp, t, c, c / groups, cp, (int)prow, front, total);
}

// the matrix-core squeeze behind its padded copy; the arguments were checked by the caller (sew_squeeze_mfma_ok included).  z: NULL, or the conv result
int ts::sew_squeeze_mfma(hipStream_t stream, const float* x, int batch, int t, int c, const void* w_taps, const float* bias, int kernel, int groups, int stride,
                         float* y, float* z, void* workspace) {
  const int cg = c / groups, t2 = t / stride;
  const long long prow = sew_prow(t, kernel, stride);
  const int rows = (SQ_TT - 1) * stride + kernel, rpp = (rows + stride - 1) / stride;
  const size_t win_lds = (size_t)stride * rpp * SQ_PITCH;
  unsigned short* const xp = static_cast<unsigned short*>(workspace);
  sew_pad16(stream, x, xp, batch, t, c, groups, prow, kernel / 2);
  SqArgs a{};
  a.xp = xp; a.w = static_cast<const unsigned short*>(w_taps); a.bias = bias; a.x = x; a.y = y; a.z = z;
  a.t = t; a.t2 = t2; a.c = c; a.cg = cg; a.cp = groups * SQ_SLOT; a.k = kernel; a.groups = groups; a.stride = stride; a.prow = (int)prow; a.rpp = rpp;
  const dim3 grid((t2 + SQ_TT - 1) / SQ_TT, (groups + 1) / 2, batch);
  if (z) hipLaunchKernelGGL(sew_squeeze_mfma_kernel<true>, grid, dim3(256), win_lds, stream, a);
  else hipLaunchKernelGGL(sew_squeeze_mfma_kernel<false>, grid, dim3(256), win_lds, stream, a);
  return hip_status(hipGetLastError());
}

extern "C" int ts_sew_abi_version(void) { return TS_SEW_ABI_VERSION; }

extern "C" int64_t ts_sew_squeeze_workspace_bytes(int32_t batch, int32_t t, int32_t c, int32_t kernel, int32_t stride, int32_t precision) {
  if (batch <= 0 || t <= 0 || c <= 0 || kernel <= 0 || stride < 1 || t < stride) return TS_EINVAL;
  if (precision < 0 || precision > 1) return TS_EUNSUPPORTED;
  // the f32 path's: conv result [B prow / s][c] f32, then the padded copy [B][prow][c] f32.  The matrix-core path's bf16 copy [B][prow][groups x 32]
  // is at most 32 / 24 x 2 bytes per element: it fits whatever the group count is
  const long long prow = sew_prow(t, kernel, stride);
  return (int64_t)batch * (prow / stride + prow) * c * (int64_t)sizeof(float);
}

extern "C" int ts_sew_squeeze_fwd(const float* x, int32_t batch, int32_t t, int32_t c, const void* w_taps, const float* bias, int32_t kernel, int32_t groups,
                                  int32_t stride, int32_t precision, float* y, void* workspace, void* stream_) {
  if (!x || !w_taps || !bias || !y || !workspace || batch <= 0 || t <= 0 || c <= 0 || kernel <= 0 || groups <= 0 || stride < 1 || t < stride || c % groups)
    return TS_EINVAL;
  if (precision < 0 || precision > 1) return TS_EUNSUPPORTED;
  if (misaligned(x) || misaligned(w_taps) || misaligned(y) || misaligned(workspace) || misaligned(bias, 3)) return TS_EUNSUPPORTED;
  const int cg = c / groups, t2 = t / stride;
  const long long prow = sew_prow(t, kernel, stride);
  if ((long long)batch * prow > 0x7fffffffll) return TS_EUNSUPPORTED;
  if (precision && (cg == 24 || cg == SQ_SLOT)) {
    if (!sew_squeeze_mfma_ok(cg, kernel, stride)) return TS_EUNSUPPORTED;
    TS_STREAM;
    return sew_squeeze_mfma(stream, x, batch, t, c, w_taps, bias, kernel, groups, stride, y, nullptr, workspace);
  }
  TS_STREAM;
  // all clips in one strided row space: output row R = sum_j xp[s R + j] W_j^T per group; clip b's frame r is row b prow / s + r, rows between clips are waste
  const long long clip_rows = prow / stride;
  float* const yp = static_cast<float*>(workspace);
  float* const xp = yp + (size_t)batch * clip_rows * c;
  hipLaunchKernelGGL(sew_pad32_kernel, dim3(nblk(prow * c), batch), dim3(256), 0, stream, x, xp, t, c, (int)prow, kernel / 2);
  const long long m = ((long long)batch * prow - kernel) / stride + 1;        // the last row whose taps stay inside the copy
  if (int st = gemm_f32(stream, false, xp, (long long)stride * c, 1, cg, c, w_taps, 1, cg, (long long)cg * cg, (long long)groups * cg * cg, yp, c, cg, false,
                        nullptr, (int)m, cg, cg, kernel, groups, false))
    return st;
  hipLaunchKernelGGL(sew_squeeze_finish_kernel, dim3(nblk((long long)t2 * c), batch), dim3(256), 0, stream, x, yp, bias, y, t, t2, c, stride, clip_rows);
  return hip_status(hipGetLastError());
}

extern "C" int ts_sew_unsqueeze_rows(const float* src, int32_t batch, int32_t t2, int32_t t, int32_t c, int32_t stride, float* dst, void* stream_) {
  if (!src || !dst || batch <= 0 || t2 <= 0 || c <= 0 || stride < 1 || (long long)t < (long long)stride * t2) return TS_EINVAL;
  if (c % 4 || misaligned(src) || misaligned(dst)) return TS_EUNSUPPORTED;
  TS_STREAM;
  const long long n_src = (long long)stride * t2 * c, n_dst = (long long)t * c;
  hipLaunchKernelGGL(sew_unsqueeze_rows_kernel, dim3(nblk(n_dst / 4), batch), dim3(256), 0, stream, src, dst, n_src, n_dst);
  return hip_status(hipGetLastError());
}
