// SEW fine-tuning in mixed precision: the squeeze (average pool + stride-s weight-normed grouped conv + GELU) of csrc/sew.hip with what its backward
// needs, time-major fp32 [B][T][C]; ABI in include/thunder_speech_amd/sew_train.h.  s = stride, k = kernel, p = k / 2, T2 = T / s.
//   ts_sew_squeeze_train_fwd   ts_sew_squeeze_fwd(precision = 1) on the same kernel (sew_squeeze_mfma_kernel<true>), which also stores the conv result z
//   ts_sew_squeeze_dgrad       dx = pool^T(dy) + conv^T(dz): per phase f = (q + p) % s a stride-1 conv of dz, sew_squeeze_dgrad_kernel
//   ts_sew_squeeze_wgrad       dw[j][g] = dz^T x(shifted by s r + j - p) over all B T2 rows, sew_squeeze_wgrad_kernel
// GELU backward and the bias gradient are ts_w2v_gelu_bwd / ts_w2v_colsum, the upsampler's zero-row padding goes back through ts_w2v_pad_rows.
#include <type_traits>

#include "w2v_rows.hpp"

#include "thunder_speech_amd/sew_train.h"
#include "sew_squeeze.hpp"

namespace ts {

// ---------------------------------------------------------------------------------------------------------------------
// Data gradient.  Input row q of a clip, with q + p = s m + f (phase f < s), receives
//     sum_u sum_o dz[m - u][o] w[f + s u][o][i]          over the taps j = f + s u < k
// -- for a fixed phase a STRIDE-1 conv over dz.  With nt = ceil(k / s) taps per phase (zero blocks where f + s u >= k), dzp = dz behind nt - 1 zero
// rows and the packed blocks Wd[f][u'] = w[f + s (nt - 1 - u')]^T, that is out_f[m] = sum_u' dzp[m + u'] Wd[f][u']: the forward's product at stride 1.
//   workgroup = 128 values of m (from p / s on: smaller m have no row q >= 0) x TWO groups of one clip; the 127 + nt rows of dzp it needs are staged ONCE in LDS (pitch 144 B, consecutive rows: the
//   conflict-free ds_read_b128 pattern of w2v_posconv_mfma_kernel) and the s phases are produced from that window one after the other, each through
//   the forward's loop: waves 2 x 2, 64 rows x one group's 32 input channels each, v_mfma_f32_32x32x16_bf16, two k-steps per tap, B = Wd blocks
//   [ci][co] straight from L2 in blocks of four taps.  MFMA work: s nt taps per 128 m = k taps per 128 output frames of the forward.
//   Epilogue of phase f: row q = s m + f - p, + dy[q / s] / s in f32 where q < s T2; rows of one phase are s C floats apart, coalesced along channels.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int SD_TB = 4;           // taps per block of prefetched weights
constexpr int SD_SB = 6;           // staging loads in flight per thread

struct SdArgs {
  const unsigned short* dzp;       // [B][prow][groups x 32] bf16, nt - 1 zero rows in front of each clip
  const unsigned short* w;         // [s][nt][groups][32 ci][32 co] bf16
  const float* dy;                 // [B][T2][C] f32 (average pool)
  float* dx;                       // [B][T][C]
  int t, t2, c, cg, cp, k, groups, stride, prow, nt, m_lo;  // m_lo = (k / 2) / stride: the first m with a row q >= 0
};

__global__ __launch_bounds__(256) void sew_squeeze_dgrad_kernel(const SdArgs a) {
  extern __shared__ __attribute__((aligned(16))) char win[];                  // [SQ_TT - 1 + nt][SQ_PITCH]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, gp = blockIdx.y, m0 = a.m_lo + blockIdx.x * SQ_TT;
  const int rows = SQ_TT - 1 + a.nt;
  const unsigned short* src = a.dzp + ((size_t)b * a.prow + m0) * a.cp + (size_t)gp * 64;
  for (int base = tid; base < rows * 8; base += 256 * SD_SB) {
    uint4 v[SD_SB];
#pragma unroll
    for (int u = 0; u < SD_SB; ++u) {
      const int chunk = base + 256 * u, r = chunk >> 3, cc = chunk & 7;
      v[u] = uint4{0u, 0u, 0u, 0u};
      if (chunk < rows * 8 && m0 + r < a.prow && gp * 64 + cc * 8 < a.cp)                                    // an odd group count: no second slot
        v[u] = *reinterpret_cast<const uint4*>(src + (size_t)r * a.cp + cc * 8);
    }
#pragma unroll
    for (int u = 0; u < SD_SB; ++u) {
      const int chunk = base + 256 * u, r = chunk >> 3, cc = chunk & 7;
      if (chunk < rows * 8) *reinterpret_cast<uint4*>(win + r * SQ_PITCH + cc * 16) = v[u];
    }
  }
  __syncthreads();
  const int wm = wave >> 1, wn = wave & 1;                                    // 64 rows x one group's 32 channels per wave
  const int g = gp * 2 + wn;
  if (g >= a.groups) return;                                                  // no barrier follows
  const int half = lane >> 5, n32 = lane & 31;
  const char* arow = win + (wm * 64 + n32) * SQ_PITCH + wn * 64 + half * 16;  // A: row = m, 8 consecutive co per k-step
  const size_t tap_stride = (size_t)a.groups * SQ_SLOT * SQ_SLOT / 8;         // uint4 units
  const int ci = g * a.cg + n32, p = a.k / 2, full = a.stride * a.t2;
  const float inv = 1.f / (float)a.stride;
  for (int f = 0; f < a.stride; ++f) {
    const uint4* wp = reinterpret_cast<const uint4*>(a.w + ((size_t)g * SQ_SLOT + n32) * SQ_SLOT + 8 * half) + (size_t)f * a.nt * tap_stride;
    f32x16 acc[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[mt][i] = 0.f;
    // the forward's weight pipeline: blocks of SD_TB taps through two register sets; loads past the last tap re-read it, nothing is multiplied by them
    uint4 b0[SD_TB][2], b1[SD_TB][2];
    auto load_taps = [&](uint4 (&bw)[SD_TB][2], int j0) {
#pragma unroll
      for (int u = 0; u < SD_TB; ++u) {
        const int j = j0 + u < a.nt ? j0 + u : a.nt - 1;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) bw[u][ks] = wp[(size_t)j * tap_stride + 2 * ks];
      }
    };
    auto run_taps = [&](const uint4 (&bw)[SD_TB][2], int j0, auto guarded) {   // guarded: the block may reach past the last tap
#pragma unroll
      for (int u = 0; u < SD_TB; ++u) {
        if (!decltype(guarded)::value || j0 + u < a.nt) {
          const char* at = arow + (j0 + u) * SQ_PITCH;
#pragma unroll
          for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
              const s16x8 af = *reinterpret_cast<const s16x8*>(at + 32 * mt * SQ_PITCH + ks * 32);
              acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, __builtin_bit_cast(s16x8, bw[u][ks]), acc[mt], 0, 0, 0);
            }
        }
      }
    };
    load_taps(b0, 0);
    int j0 = 0;
    for (; j0 + 2 * SD_TB <= a.nt; j0 += 2 * SD_TB) {
      load_taps(b1, j0 + SD_TB);
      run_taps(b0, j0, std::false_type{});
      load_taps(b0, j0 + 2 * SD_TB);
      run_taps(b1, j0 + SD_TB, std::false_type{});
    }
    if (j0 < a.nt) {
      load_taps(b1, j0 + SD_TB);
      run_taps(b0, j0, std::true_type{});
      run_taps(b1, j0 + SD_TB, std::true_type{});
    }
    if (n32 < a.cg) {                                                         // (the zero channels of a 24-channel group are not stored)
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int m = m0 + wm * 64 + 32 * mt + 8 * (i >> 2) + 4 * half + (i & 3);
          const long long q = (long long)m * a.stride + f - p;
          if (q >= 0 && q < a.t) {
            float v = acc[mt][i];
            if (q < full) v += a.dy[((size_t)b * a.t2 + (size_t)(q / a.stride)) * a.c + ci] * inv;
            a.dx[((size_t)b * a.t + (size_t)q) * a.c + ci] = v;
          }
        }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Weight gradient: for one (tap j, group g) a 32 x 32 product contracted over all B T2 output frames r,
//     dw[j][g][o][i] = sum_b sum_r dz[b][r][o] xp[b][s r + j][i],        xp = x behind p zero rows per clip (the forward's padded copy)
// -- the scheme of w2v_posconv_wgrad_kernel.  Workgroup = (8 taps, pair of groups); a stage is tt output frames of one clip: the dz tile [tt][64] and the
// xp window of s (tt - 1) + 8 rows (shared by the eight taps) in LDS as bf16.  The window is stored split by phase as the forward's -- row u at slot
// (u % s) rpw + u / s -- so that the rows s r + jj of one tap are CONSECUTIVE slots and both operands come out of LDS with the transposing reads
// (rows = the contraction index r).  Wave = one group x four taps, v_mfma_f32_32x32x16_bf16, 64 f32 accumulators per lane; the next stage's rows
// travel global -> registers while the current one is multiplied.  Each workgroup owns its outputs: no partials, no atomics.
// tt = the largest multiple of 32 up to 128 whose tile + window fit 64 KiB (128 at s <= 2, 96 at s = 3).
// ---------------------------------------------------------------------------------------------------------------------
constexpr int SW_TAPS = 8;
constexpr int SW_RZ = 4, SW_RX = 10;   // 16-byte chunks per thread of the dz tile (128 x 8 / 256) and of the window (up to 2 560)

struct SwArgs {
  const unsigned short* dz;        // [B][T2][groups x 32] bf16
  const unsigned short* xp;        // [B][prow][groups x 32] bf16, p zero rows in front of each clip
  float* dw;                       // [k][groups][cg][cg]
  int batch, t2, cg, cp, k, groups, stride, prow, tt, rpw;
};

__global__ __launch_bounds__(256) void sew_squeeze_wgrad_kernel(const SwArgs a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  char* const dzs = lds;                                        // [tt][SQ_PITCH]
  char* const xps = lds + a.tt * SQ_PITCH;                      // [stride][rpw][SQ_PITCH]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j0 = blockIdx.x * SW_TAPS, gp = blockIdx.y;
  const int n_ch = (a.t2 + a.tt - 1) / a.tt, S = a.batch * n_ch;
  const int wrows = a.stride * (a.tt - 1) + SW_TAPS;            // window rows of a stage
  f32x16 acc[4];
#pragma unroll
  for (int tp = 0; tp < 4; ++tp)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[tp][r] = 0.f;
  uint4 rz[SW_RZ], rx[SW_RX];
  // Every load of a stage is issued whatever its guard says -- a chunk outside the clip, the window or the copy reads the copy's first 16 bytes --
  // and the guard is applied when the chunk is written to LDS: guarded loads are branches, and the compiler put waits for the loads in flight
  // between them, i.e. a memory round trip in front of every stage's MFMAs.
  auto dz_ok = [&](int r0, int r, int cc) { return r < a.tt && r0 + r < a.t2 && gp * 64 + cc * 8 < a.cp; };
  auto x_ok = [&](int r0, int u, int cc) { return u < wrows && (long long)r0 * a.stride + j0 + u < a.prow && gp * 64 + cc * 8 < a.cp; };
  auto fetch = [&](int st) {
    const int b = st / n_ch, r0 = (st % n_ch) * a.tt;
#pragma unroll
    for (int q = 0; q < SW_RZ; ++q) {
      const int chunk = tid + 256 * q, r = chunk >> 3, cc = chunk & 7;
      const size_t off = dz_ok(r0, r, cc) ? ((size_t)b * a.t2 + r0 + r) * a.cp + (size_t)gp * 64 + cc * 8 : 0;
      rz[q] = *reinterpret_cast<const uint4*>(a.dz + off);
    }
#pragma unroll
    for (int q = 0; q < SW_RX; ++q) {
      const int chunk = tid + 256 * q, u = chunk >> 3, cc = chunk & 7;
      const long long row = (long long)r0 * a.stride + j0 + u;  // row of the clip's padded copy
      const size_t off = x_ok(r0, u, cc) ? ((size_t)b * a.prow + (size_t)row) * a.cp + (size_t)gp * 64 + cc * 8 : 0;
      rx[q] = *reinterpret_cast<const uint4*>(a.xp + off);
    }
  };
  auto stage = [&](int st) {
    const int r0 = (st % n_ch) * a.tt;
    auto keep = [](const uint4& v, bool ok) { const unsigned m = ok ? 0xffffffffu : 0u; return uint4{v.x & m, v.y & m, v.z & m, v.w & m}; };
#pragma unroll
    for (int q = 0; q < SW_RZ; ++q) {
      const int chunk = tid + 256 * q, r = chunk >> 3, cc = chunk & 7;
      if (r < a.tt) *reinterpret_cast<uint4*>(dzs + r * SQ_PITCH + cc * 16) = keep(rz[q], dz_ok(r0, r, cc));
    }
#pragma unroll
    for (int q = 0; q < SW_RX; ++q) {
      const int chunk = tid + 256 * q, u = chunk >> 3, cc = chunk & 7;
      const int slot = u / a.stride, ph = u - slot * a.stride;
      if (u < wrows) *reinterpret_cast<uint4*>(xps + (ph * a.rpw + slot) * SQ_PITCH + cc * 16) = keep(rx[q], x_ok(r0, u, cc));
    }
  };
  const int half = lane >> 5, q4 = (lane >> 2) & 3, gq = (lane >> 4) & 1, p4 = lane & 3;
  const int gi = wave & 1, jb = 4 * (wave >> 1);                              // this wave: group gi of the pair, taps j0 + jb .. + 3
  const int tr_off = (8 * half + q4) * SQ_PITCH + (16 * gq + 4 * p4) * 2 + 64 * gi;       // transposing read: rows = contraction index, columns = M / N index
  auto tr8 = [&](const char* ptr) {
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((TS_LDS s16x4*)((TS_LDS char*)ptr));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((TS_LDS s16x4*)((TS_LDS char*)ptr + 4 * SQ_PITCH));
    return s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  };
  int xoff[4];                                                                // tap jj = jb + tp: phase jj % s, first slot jj / s
#pragma unroll
  for (int tp = 0; tp < 4; ++tp) {
    const int jj = jb + tp, slot = jj / a.stride, ph = jj - slot * a.stride;
    xoff[tp] = (ph * a.rpw + slot) * SQ_PITCH + tr_off;
  }
  if (S > 0) fetch(0);
  for (int st = 0; st < S; ++st) {
    __syncthreads();                                       // the previous stage has been multiplied
    stage(st);
    __syncthreads();
    if (st + 1 < S) fetch(st + 1);
    // the fragments of k-step ks + 1 are read while ks is multiplied, through two register sets (tt is a launch argument: the loop is not unrolled,
    // and with the reads inside the step every step would wait out an LDS round trip in front of its four MFMAs).  tt / 16 is even.
    const int n_ks = a.tt / 16;
    s16x8 a0 = tr8(dzs + tr_off), b0[4], a1, b1[4];
#pragma unroll
    for (int tp = 0; tp < 4; ++tp) b0[tp] = tr8(xps + xoff[tp]);
    for (int ks = 0; ks < n_ks; ks += 2) {
      a1 = tr8(dzs + 16 * (ks + 1) * SQ_PITCH + tr_off);
#pragma unroll
      for (int tp = 0; tp < 4; ++tp) b1[tp] = tr8(xps + 16 * (ks + 1) * SQ_PITCH + xoff[tp]);
#pragma unroll
      for (int tp = 0; tp < 4; ++tp) acc[tp] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0[tp], acc[tp], 0, 0, 0);
      const int nx = ks + 2 < n_ks ? ks + 2 : ks;             // (the last pair re-reads its own rows: in bounds, not multiplied)
      a0 = tr8(dzs + 16 * nx * SQ_PITCH + tr_off);
#pragma unroll
      for (int tp = 0; tp < 4; ++tp) b0[tp] = tr8(xps + 16 * nx * SQ_PITCH + xoff[tp]);
#pragma unroll
      for (int tp = 0; tp < 4; ++tp) acc[tp] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1[tp], acc[tp], 0, 0, 0);
    }
  }
  // accumulator register r: o = (r & 3) + 8 (r >> 2) + 4 half, i = lane % 32; the padded lanes of a 24-channel group are not stored
  const int g = gp * 2 + gi, i = lane & 31;
  if (g >= a.groups || i >= a.cg) return;
#pragma unroll
  for (int tp = 0; tp < 4; ++tp) {
    const int j = j0 + jb + tp;
    if (j >= a.k) continue;
    float* const out = a.dw + ((size_t)j * a.groups + g) * a.cg * a.cg;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int o = (r & 3) + 8 * (r >> 2) + 4 * half;
      if (o < a.cg) out[(size_t)o * a.cg + i] = acc[tp][r];
    }
  }
}

// frames per stage of the weight gradient: the largest multiple of 32 (an even number of k-steps) up to 128 with tile + window within 64 KiB; 0: none
static inline int sw_stage_frames(int stride) {
  for (int tt = 128; tt >= 32; tt -= 32)
    if ((size_t)(tt + (long long)stride * (tt + SW_TAPS)) * SQ_PITCH <= SQ_LDS_MAX && ((long long)stride * (tt - 1) + SW_TAPS) * 8 <= 256 * SW_RX) return tt;
  return 0;
}

// the checks the three launches share, behind their NULL checks: TS_EINVAL, then TS_EUNSUPPORTED outside the support matrix, else 0
static inline int sq_train_check(int batch, int t, int c, int kernel, int groups, int stride) {
  if (batch <= 0 || t <= 0 || c <= 0 || kernel <= 0 || groups <= 0 || stride < 1 || t < stride || c % groups) return TS_EINVAL;
  if (!sew_squeeze_mfma_ok(c / groups, kernel, stride) || !sw_stage_frames(stride)) return TS_EUNSUPPORTED;
  if ((long long)batch * sew_prow(t, kernel, stride) > 0x7fffffffll) return TS_EUNSUPPORTED;
  return 0;
}

}  // namespace ts

using namespace ts;

extern "C" int ts_sew_train_abi_version(void) { return TS_SEW_TRAIN_ABI_VERSION; }

extern "C" int ts_sew_squeeze_train_supported(int32_t batch, int32_t t, int32_t c, int32_t kernel, int32_t groups, int32_t stride) {
  return sq_train_check(batch, t, c, kernel, groups, stride);
}

extern "C" int ts_sew_squeeze_train_fwd(const float* x, int32_t batch, int32_t t, int32_t c, const void* w_taps, const float* bias, int32_t kernel,
                                        int32_t groups, int32_t stride, float* y, float* z, void* workspace, void* stream_) {
  if (!x || !w_taps || !bias || !y || !z || !workspace) return TS_EINVAL;
  if (int st = sq_train_check(batch, t, c, kernel, groups, stride)) return st;
  if (misaligned(x) || misaligned(w_taps) || misaligned(y) || misaligned(z) || misaligned(workspace) || misaligned(bias, 3)) return TS_EUNSUPPORTED;
  TS_STREAM;
  return sew_squeeze_mfma(stream, x, batch, t, c, w_taps, bias, kernel, groups, stride, y, z, workspace);
}

extern "C" int64_t ts_sew_squeeze_dgrad_workspace_bytes(int32_t batch, int32_t t, int32_t c, int32_t kernel, int32_t stride) {
  if (batch <= 0 || t <= 0 || c <= 0 || kernel <= 0 || stride < 1 || t < stride) return TS_EINVAL;
  // the bf16 copy [B][T2 + nt][groups x 32] is at most 32 / 24 x 2 bytes per element of [B][T2 + nt][c]
  const long long nt = (kernel + stride - 1) / stride;
  return (int64_t)batch * (t / stride + nt) * c * (int64_t)sizeof(float);
}

extern "C" int ts_sew_squeeze_dgrad(const float* dz, const float* dy, int32_t batch, int32_t t, int32_t c, const void* w_dgrad, int32_t kernel, int32_t groups,
                                    int32_t stride, float* dx, void* workspace, void* stream_) {
  if (!dz || !dy || !w_dgrad || !dx || !workspace) return TS_EINVAL;
  if (int st = sq_train_check(batch, t, c, kernel, groups, stride)) return st;
  if (misaligned(dz) || misaligned(dy) || misaligned(w_dgrad) || misaligned(dx) || misaligned(workspace)) return TS_EUNSUPPORTED;
  TS_STREAM;
  const int t2 = t / stride, nt = (kernel + stride - 1) / stride, prow = t2 + nt;
  unsigned short* const dzp = static_cast<unsigned short*>(workspace);
  sew_pad16(stream, dz, dzp, batch, t2, c, groups, prow, nt - 1);
  SdArgs a{};
  a.dzp = dzp; a.w = static_cast<const unsigned short*>(w_dgrad); a.dy = dy; a.dx = dx;
  a.t = t; a.t2 = t2; a.c = c; a.cg = c / groups; a.cp = groups * SQ_SLOT; a.k = kernel; a.groups = groups; a.stride = stride; a.prow = prow; a.nt = nt;
  // (q + p) / s over the t input rows runs from p / s to (t - 1 + p) / s: tiles start at p / s, so that t = s x 128 n rows are n tiles as in the forward
  a.m_lo = (kernel / 2) / stride;
  const int m = (t - 1 + kernel / 2) / stride + 1 - a.m_lo;
  hipLaunchKernelGGL(sew_squeeze_dgrad_kernel, dim3((m + SQ_TT - 1) / SQ_TT, (groups + 1) / 2, batch), dim3(256), (size_t)(SQ_TT - 1 + nt) * SQ_PITCH, stream, a);
  return hip_status(hipGetLastError());
}

extern "C" int64_t ts_sew_squeeze_wgrad_workspace_bytes(int32_t batch, int32_t t, int32_t c, int32_t kernel, int32_t stride) {
  if (batch <= 0 || t <= 0 || c <= 0 || kernel <= 0 || stride < 1 || t < stride) return TS_EINVAL;
  // bf16 copies [B][prow][groups x 32] of x and [B][T2][groups x 32] of dz, each at most 32 / 24 x 2 bytes per f32 element
  return (int64_t)batch * (sew_prow(t, kernel, stride) + t / stride) * c * (int64_t)sizeof(float);
}

extern "C" int ts_sew_squeeze_wgrad(const float* dz, const float* x, int32_t batch, int32_t t, int32_t c, int32_t kernel, int32_t groups, int32_t stride,
                                    float* dw, void* workspace, void* stream_) {
  if (!dz || !x || !dw || !workspace) return TS_EINVAL;
  if (int st = sq_train_check(batch, t, c, kernel, groups, stride)) return st;
  if (misaligned(dz) || misaligned(x) || misaligned(dw) || misaligned(workspace)) return TS_EUNSUPPORTED;
  TS_STREAM;
  const int t2 = t / stride, cp = groups * SQ_SLOT, tt = sw_stage_frames(stride);
  const long long prow = sew_prow(t, kernel, stride);
  unsigned short* const xp = static_cast<unsigned short*>(workspace);
  unsigned short* const dz16 = xp + (size_t)batch * prow * cp;
  sew_pad16(stream, x, xp, batch, t, c, groups, prow, kernel / 2);
  sew_pad16(stream, dz, dz16, batch, t2, c, groups, t2, 0);
  SwArgs a{};
  a.dz = dz16; a.xp = xp; a.dw = dw;
  a.batch = batch; a.t2 = t2; a.cg = c / groups; a.cp = cp; a.k = kernel; a.groups = groups; a.stride = stride; a.prow = (int)prow; a.tt = tt; a.rpw = tt + SW_TAPS;
  const size_t lds = (size_t)(tt + stride * (tt + SW_TAPS)) * SQ_PITCH;
  hipLaunchKernelGGL(sew_squeeze_wgrad_kernel, dim3((kernel + SW_TAPS - 1) / SW_TAPS, (groups + 1) / 2), dim3(256), lds, stream, a);
  return hip_status(hipGetLastError());
}
