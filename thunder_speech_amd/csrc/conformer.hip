// The conformer block of wav2vec2-conformer with rotary position embeddings (transformers modeling_wav2vec2_conformer.py, reached from
// huggingface/compatibility.py:31-42 for a wav2vec2-conformer checkpoint).  Declared in include/thunder_speech_amd/conformer.h.
//
//   ts_conformer_glu_dwconv_fwd        act(BN(dwconv(GLU(u)))): a tile of GLU'd frames and its (KT - 1)-frame halo staged in LDS as f32,
//                                      each lane one channel and a run of 32 output frames, taps and weights in registers
//   ts_conformer_layernorm_rotary_fwd  LN(x) and its rotary-rotated copy from one read of the row (w2v_layernorm_kernel's layout)
//   ts_conformer_linear_fwd            the bf16 GEMM of csrc/gemm_nt.hip with its GELU / SiLU epilogue, column slices of a wider output;
//                                      f32: the f32 GEMM and one epilogue pass
#include "w2v_rows.hpp"
#include "thunder_speech_amd/conformer.h"

namespace ts {

namespace {

// act 1: GELU (erf), 2: SiLU (swish), else identity
__device__ __forceinline__ float act_cf(float x, int act) {
  if (act == 1) return gelu_erf(x);
  if (act == 2) return silu(x);
  return x;
}
__device__ __forceinline__ float glu_cf(float a, float g) { return a / (1.f + __expf(-g)); }

// ---------------------------------------------------------------------------------------------------------------------
// GLU + depthwise conv + folded BatchNorm + activation
// ---------------------------------------------------------------------------------------------------------------------
constexpr int GD_CW = 64;               // channels per workgroup: lane = channel
constexpr int GD_FPT = 32;              // output frames per thread
constexpr int GD_TF = 4 * GD_FPT;       // output frames per workgroup (4 waves)
constexpr int GD_FC = 16;               // frames per unrolled chunk of a thread's run

// KT: the odd tap count the kernel is compiled for; a kernel k < KT runs with its taps centred in KT and (KT - k) / 2 zero taps on either
// side, which is the same convolution (padding (KT - 1) / 2 instead of (k - 1) / 2); KT = 63 loops over the k real taps instead.  Workgroup = (128 output frames, 64 channels, clip).
//  1. stage: rows f0 - P .. f0 + 127 + P of the clip (P = (KT - 1) / 2), GLU'd into f32 LDS [rows][64] -- 8 lanes per row, 8 channels per
//     lane (16-byte loads of each half); frames outside [0, t) are 0.  GLU runs once per staged element (the halo: (KT - 1) / 128 more).
//  2. convolve: wave w, lane l owns channel c0 + l and output frames f0 + 32 w .. + 31, taps in registers; per chunk of 16 frames the loop
//     over its 16 + KT - 1 staged rows is unrolled, each row read once from LDS (consecutive lanes, consecutive banks) and multiplied into
//     every accumulator it reaches.
template <int KT, bool BF16>
__global__ __launch_bounds__(256) void conformer_glu_dwconv_kernel(const void* __restrict__ u_, int t, int c, const float* __restrict__ dw_w, int k,
                                                                   const float* __restrict__ bn_scale, const float* __restrict__ bn_shift, int act,
                                                                   void* __restrict__ y_) {
  constexpr int P = (KT - 1) / 2;
  constexpr int ROWS = GD_TF + KT - 1;
  __shared__ __attribute__((aligned(16))) float g[ROWS][GD_CW];
  const int tid = threadIdx.x;
  const int b = blockIdx.z, f0 = blockIdx.x * GD_TF, c0 = blockIdx.y * GD_CW;
  {
    const int q = tid & 7, ch = c0 + 8 * q;
    for (int r = tid >> 3; r < ROWS; r += 32) {
      const int f = f0 - P + r;
      f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
      if (f >= 0 && f < t && ch < c) {
        const size_t base = ((size_t)b * t + f) * 2 * c + ch;
        if constexpr (BF16) {
          const unsigned short* u = static_cast<const unsigned short*>(u_);
          const u32x4 av = *reinterpret_cast<const u32x4*>(u + base);
          const u32x4 gv = *reinterpret_cast<const u32x4*>(u + base + c);
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            lo[2 * i] = glu_cf(bf16_lo(av[i]), bf16_lo(gv[i]));
            lo[2 * i + 1] = glu_cf(bf16_hi(av[i]), bf16_hi(gv[i]));
            hi[2 * i] = glu_cf(bf16_lo(av[2 + i]), bf16_lo(gv[2 + i]));
            hi[2 * i + 1] = glu_cf(bf16_hi(av[2 + i]), bf16_hi(gv[2 + i]));
          }
        } else {
          const float* u = static_cast<const float*>(u_);
          const f32x4 a0 = *reinterpret_cast<const f32x4*>(u + base), a1 = *reinterpret_cast<const f32x4*>(u + base + 4);
          const f32x4 g0 = *reinterpret_cast<const f32x4*>(u + base + c), g1 = *reinterpret_cast<const f32x4*>(u + base + c + 4);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            lo[i] = glu_cf(a0[i], g0[i]);
            hi[i] = glu_cf(a1[i], g1[i]);
          }
        }
      }
      *reinterpret_cast<f32x4*>(&g[r][8 * q]) = lo;
      *reinterpret_cast<f32x4*>(&g[r][8 * q + 4]) = hi;
    }
  }
  __syncthreads();
  const int lane = tid & 63, wv = tid >> 6;
  const int ch = c0 + lane, fs = f0 + wv * GD_FPT;
  if (ch >= c || fs >= t) return;                  // nothing below synchronises
  const int off = (KT - k) / 2;
  const float sc = bn_scale[ch], sh = bn_shift[ch];
  float w[KT <= 31 ? KT : 1];
  if constexpr (KT <= 31) {
#pragma unroll
    for (int j = 0; j < KT; ++j) w[j] = (j >= off && j < off + k) ? dw_w[(size_t)(j - off) * c + ch] : 0.f;
  }
  // the run in chunks of GD_FC frames: a chunk's (GD_FC + KT - 1) x GD_FC tap loop unrolls completely (the whole run's does not), so every
  // w[j] is a register and every staged row of the chunk is read once
#pragma unroll 1
  for (int f0c = 0; f0c < GD_FPT && fs + f0c < t; f0c += GD_FC) {
    float acc[GD_FC];
#pragma unroll
    for (int f = 0; f < GD_FC; ++f) acc[f] = 0.f;
    const int r0 = wv * GD_FPT + f0c;
    if constexpr (KT <= 31) {
#pragma unroll
      for (int s = 0; s < GD_FC + KT - 1; ++s) {
        const float v = g[r0 + s][lane];
#pragma unroll
        for (int f = 0; f < GD_FC; ++f) {
          const int j = s - f;
          if (j >= 0 && j < KT) acc[f] = fmaf(w[j], v, acc[f]);
        }
      }
    } else {
      // 31 < k <= 63 (no published checkpoint): taps in a loop, one LDS read per tap and frame
      for (int j = 0; j < k; ++j) {
        const float wj = dw_w[(size_t)j * c + ch];
#pragma unroll
        for (int f = 0; f < GD_FC; ++f) acc[f] = fmaf(wj, g[r0 + off + j + f][lane], acc[f]);
      }
    }
    const size_t ybase = ((size_t)b * t + fs + f0c) * c + ch;
#pragma unroll
    for (int f = 0; f < GD_FC; ++f) {
      if (fs + f0c + f < t) {
        const float v = act_cf(fmaf(sc, acc[f], sh), act);
        if constexpr (BF16) static_cast<unsigned short*>(y_)[ybase + (size_t)f * c] = (unsigned short)(pack_bf16(v, 0.f) & 0xffffu);
        else static_cast<float*>(y_)[ybase + (size_t)f * c] = v;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// LayerNorm + rotary copy
// ---------------------------------------------------------------------------------------------------------------------
// One wavefront per row, NV float4 per lane (w2v_layernorm_kernel's layout: lane l of chunk it holds channels 256 it + 4 l .. + 3).  A head of
// 64 channels is 16 lanes; channel j + 32 of a head lives 8 lanes after channel j, so rotate_half is one lane exchange (xor 8), and lane l
// needs the frequencies 4 (l & 7) .. + 3 of the row's position: one float4 of cos and one of sin for the whole row.
template <int NV, bool BF16>
__global__ __launch_bounds__(256) void conformer_ln_rotary_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                                  float eps, long long rows, int t, int c, const float* __restrict__ cos_sin, int t_table,
                                                                  void* __restrict__ y_, void* __restrict__ yr_) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;                         // wave-uniform: the exchanges below see whole waves
  const float* xr = x + row * c;
  f32x4 v[NV];
  float s = 0.f;
#pragma unroll
  for (int it = 0; it < NV; ++it) {
    const int i = (it * 64 + lane) * 4;
    v[it] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (i < c) {
      v[it] = *reinterpret_cast<const f32x4*>(xr + i);
      s += (v[it][0] + v[it][1]) + (v[it][2] + v[it][3]);
    }
  }
  const float mu = wave_sum(s) / c;
  float q = 0.f;
#pragma unroll
  for (int it = 0; it < NV; ++it) {
    const int i = (it * 64 + lane) * 4;
    if (i < c) {
      const float d0 = v[it][0] - mu, d1 = v[it][1] - mu, d2 = v[it][2] - mu, d3 = v[it][3] - mu;
      q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    }
  }
  const float rs = rsqrtf(wave_sum(q) / c + eps);
  const int pos = (int)(row % t);
  const f32x4 cv = *reinterpret_cast<const f32x4*>(cos_sin + (size_t)pos * 32 + 4 * (lane & 7));
  const f32x4 sv = *reinterpret_cast<const f32x4*>(cos_sin + ((size_t)t_table + pos) * 32 + 4 * (lane & 7));
  const float sgn = (lane & 8) ? 1.f : -1.f;
#pragma unroll
  for (int it = 0; it < NV; ++it) {
    const int i = (it * 64 + lane) * 4;
    f32x4 o4 = {0.f, 0.f, 0.f, 0.f};
    if (i < c) {
      const f32x4 w4 = *reinterpret_cast<const f32x4*>(w + i), b4 = *reinterpret_cast<const f32x4*>(b + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) o4[e] = (v[it][e] - mu) * rs * w4[e] + b4[e];
    }
    f32x4 r4;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float p = __shfl_xor(o4[e], 8);        // every lane of the wave takes part (c % 64 == 0: a head's 16 lanes are valid together)
      r4[e] = o4[e] * cv[e] + (sgn * p) * sv[e];
    }
    if (i < c) {
      if constexpr (BF16) {
        *reinterpret_cast<u32x2*>(static_cast<unsigned short*>(y_) + row * c + i) = u32x2{pack_bf16(o4[0], o4[1]), pack_bf16(o4[2], o4[3])};
        *reinterpret_cast<u32x2*>(static_cast<unsigned short*>(yr_) + row * c + i) = u32x2{pack_bf16(r4[0], r4[1]), pack_bf16(r4[2], r4[3])};
      } else {
        *reinterpret_cast<f32x4*>(static_cast<float*>(y_) + row * c + i) = o4;
        *reinterpret_cast<f32x4*>(static_cast<float*>(yr_) + row * c + i) = r4;
      }
    }
  }
}

// f32 epilogue of ts_conformer_linear_fwd: y[r][col] = act(y[r][col] + bias[col]) (+ res[r][col]), four columns per thread
__global__ __launch_bounds__(256) void conformer_bias_act_kernel(float* __restrict__ y, long long ldc, const float* __restrict__ bias,
                                                                 const float* __restrict__ res, long long ld_res, long long rows, int n, int act) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const int n4 = n >> 2;
  if (idx >= rows * n4) return;
  const long long r = idx / n4;
  const int col = (int)(idx - r * n4) * 4;
  f32x4 v = *reinterpret_cast<const f32x4*>(y + r * ldc + col);
  if (bias) v += *reinterpret_cast<const f32x4*>(bias + col);
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = act_cf(v[e], act);
  if (res) v += *reinterpret_cast<const f32x4*>(res + r * ld_res + col);
  *reinterpret_cast<f32x4*>(y + r * ldc + col) = v;
}

}  // namespace
}  // namespace ts

using namespace ts;

extern "C" int ts_conformer_abi_version(void) { return TS_CONFORMER_ABI_VERSION; }

extern "C" int ts_conformer_glu_dwconv_fwd(const void* u, int32_t batch, int32_t t, int32_t c, const float* dw_w, int32_t kernel, const float* bn_scale,
                                           const float* bn_shift, int32_t act, int32_t precision, void* y, void* stream_) {
  if (!u || !dw_w || !bn_scale || !bn_shift || !y || batch <= 0 || t <= 0 || c <= 0) return TS_EINVAL;
  if (kernel < 1 || kernel > 63 || !(kernel & 1) || c % 8 || misaligned(u) || (act != 1 && act != 2) || precision < 0 || precision > 1 || batch > 65535)
    return TS_EUNSUPPORTED;
  TS_STREAM;
  const dim3 grid((unsigned)((t + GD_TF - 1) / GD_TF), (unsigned)((c + GD_CW - 1) / GD_CW), (unsigned)batch);
#define TS_GD(KT_)                                                                                                                       \
  do {                                                                                                                                   \
    if (precision) hipLaunchKernelGGL((conformer_glu_dwconv_kernel<KT_, true>), grid, dim3(256), 0, stream, u, t, c, dw_w, kernel, bn_scale, \
                                      bn_shift, act, y);                                                                                 \
    else hipLaunchKernelGGL((conformer_glu_dwconv_kernel<KT_, false>), grid, dim3(256), 0, stream, u, t, c, dw_w, kernel, bn_scale,      \
                            bn_shift, act, y);                                                                                           \
  } while (0)
  if (kernel <= 3) TS_GD(3);
  else if (kernel <= 7) TS_GD(7);
  else if (kernel <= 15) TS_GD(15);
  else if (kernel <= 31) TS_GD(31);
  else TS_GD(63);
#undef TS_GD
  return hip_status(hipGetLastError());
}

extern "C" int ts_conformer_layernorm_rotary_fwd(const float* x, const float* w, const float* b, float eps, int32_t batch, int32_t t, int32_t c,
                                                 int32_t heads, const float* cos_sin, int32_t t_table, int32_t precision, void* y, void* y_rot,
                                                 void* stream_) {
  if (!x || !w || !b || !cos_sin || !y || !y_rot || batch <= 0 || t <= 0 || t > t_table) return TS_EINVAL;
  if (heads <= 0 || c != 64 * heads || c > 4096 || precision < 0 || precision > 1) return TS_EUNSUPPORTED;
  if (misaligned(x) || misaligned(w) || misaligned(b) || misaligned(cos_sin) || misaligned(y, 7) || misaligned(y_rot, 7) ||
      (!precision && (misaligned(y) || misaligned(y_rot))))
    return TS_EUNSUPPORTED;
  TS_STREAM;
  const long long rows = (long long)batch * t;
  const dim3 grid((unsigned)((rows + 3) / 4));
#define TS_LNR(NV_)                                                                                                                             \
  do {                                                                                                                                          \
    if (precision) hipLaunchKernelGGL((conformer_ln_rotary_kernel<NV_, true>), grid, dim3(256), 0, stream, x, w, b, eps, rows, t, c, cos_sin,   \
                                      t_table, y, y_rot);                                                                                       \
    else hipLaunchKernelGGL((conformer_ln_rotary_kernel<NV_, false>), grid, dim3(256), 0, stream, x, w, b, eps, rows, t, c, cos_sin, t_table,  \
                            y, y_rot);                                                                                                          \
  } while (0)
  if (c <= 256) TS_LNR(1); else if (c <= 512) TS_LNR(2); else if (c <= 1024) TS_LNR(4); else if (c <= 2048) TS_LNR(8); else TS_LNR(16);
#undef TS_LNR
  return hip_status(hipGetLastError());
}

extern "C" int ts_conformer_linear_fwd(const void* x, int64_t lda, const void* w, const void* w_frag, const float* bias, const float* res, int64_t ld_res,
                                       float* y, int64_t ldc, void* y_op, int64_t ld_op, int64_t rows, int32_t n, int32_t k, int32_t act, int32_t precision,
                                       void* stream_) {
  if (!x || !w || rows <= 0 || n <= 0 || k <= 0 || lda < k || (y && ldc < n) || (y_op && ld_op < n) || (res && ld_res < n)) return TS_EINVAL;
  if (act < 0 || act > 2 || precision < 0 || precision > 1) return TS_EUNSUPPORTED;
  TS_STREAM;
  if (precision) {
    if (!y && !y_op) return TS_EINVAL;
    return gemm_nt_bf16_act(stream, x, lda, 0, w, k, bias, res, ld_res, y, ldc, y_op, ld_op, 0, rows, n, k, act, 1, w_frag);
  }
  if (!y || y_op) return TS_EINVAL;                 // f32: the f32 result is the operand of the next product
  if (n % 4 || ldc % 4 || misaligned(y) || (res && (ld_res % 4 || misaligned(res))) || (bias && misaligned(bias))) return TS_EUNSUPPORTED;
  // res == y: accumulate into the residual stream in place (beta = 1 inside the GEMM); the activation comes before the residual, so an
  // activated product needs a result buffer of its own
  const bool inplace = res && static_cast<const void*>(res) == static_cast<const void*>(y) && ld_res == ldc;
  if (inplace && act) return TS_EUNSUPPORTED;
  if (int st = gemm_f32(stream, false, x, lda, 1, 0, 0, w, 1, k, 0, 0, y, ldc, 0, false, nullptr, (int)rows, n, k, 1, 1, inplace)) return st;
  const float* res_e = inplace ? nullptr : res;
  if (bias || res_e || act)
    hipLaunchKernelGGL(conformer_bias_act_kernel, dim3(nblk(rows * (n / 4))), dim3(256), 0, stream, y, (long long)ldc, bias, res_e,
                       (long long)ld_res, (long long)rows, n, act);
  return hip_status(hipGetLastError());
}
