// Fine-tuning of the rotary wav2vec2-conformer (transformers modeling_wav2vec2_conformer.py in train mode): what the wav2vec2 training kernels
// (csrc/w2v_train.hip, w2v_attn_train.hip, gemm_nt.hip) do not cover.  Declared in include/thunder_speech_amd/conformer_train.h.
//
//   ts_conformer_glu_dwconv_train_fwd   z = dwconv(GLU(u)), unnormalised, + per-workgroup (count, mean, M2) of z per channel (float64): the
//                                       staging and tap loop of conformer_glu_dwconv_kernel (csrc/conformer.hip)
//   ts_conformer_bn_stats               Chan's combine of those partials in float64, workgroup order -> mean, rstd, biased variance
//   ts_conformer_bn_act_cast            act(BN(z)) straight to the bf16 operands of pointwise_conv2 (ffn_act_cast_kernel's tiles)
//   ts_conformer_bn_act_bwd_sums        d gamma, d beta: partials per 32 rows, ordered finish
//   ts_conformer_glu_dwconv_train_bwd   dz for a tile and its halo staged in LDS (never stored); the transposed conv and the weight gradient
//                                       read the same staged rows; GLU backward from a recomputed gate; ordered finish of d dw_w
//   ts_conformer_rotary_bwd             transpose of the rotary rotation + the value branch's gradient
//   ts_conformer_ffn_act_cast / _bwd    the feed-forward activation pair by act code (act 1: the wav2vec2 pair's own launches)
// No atomics; every sum has a fixed order.
#include "w2v_rows.hpp"
#include "ts_philox.hpp"
#include "thunder_speech_amd/conformer_train.h"

namespace ts {

namespace {

constexpr int CT_CW = 64;               // channels per workgroup: lane = channel
constexpr int CT_FPT = 32;              // frames per thread
constexpr int CT_TF = 4 * CT_FPT;       // frames per workgroup (4 waves)
constexpr int CT_SR = 32;               // rows per workgroup of the d gamma / d beta partials

__device__ __forceinline__ float sigmoid_ct(float x) { return 1.f / (1.f + __expf(-x)); }
__device__ __forceinline__ float act_ct(float y, int act) { return act == 1 ? gelu_erf(y) : silu(y); }
__device__ __forceinline__ float dact_ct(float y, int act) {
  if (act == 1) return 0.5f * (1.f + erf_as(y * 0.70710678118654752f)) + y * 0.3989422804014327f * __expf(-0.5f * y * y);
  const float s = sigmoid_ct(y);
  return s * (1.f + y * (1.f - s));
}

// ---------------------------------------------------------------------------------------------------------------------
// forward: GLU + depthwise conv, and the BatchNorm partials
// ---------------------------------------------------------------------------------------------------------------------
// conformer_glu_dwconv_kernel (csrc/conformer.hip) for f32 input without its epilogue: KT, the staging and the tap loop are that kernel's.
// Every thread then sums its up to 32 outputs and their squares in float64; the four waves' sums meet in LDS and wave 0 writes, per channel,
// (count, mean, centred sum of squares) of the workgroup's frames: part[wg][3][c], wg = clip * tiles + tile.
template <int KT>
__global__ __launch_bounds__(256) void ct_glu_dwconv_fwd_kernel(const float* __restrict__ u, int t, int c, const float* __restrict__ dw_w, int k,
                                                                float* __restrict__ z, double* __restrict__ part) {
  constexpr int P = (KT - 1) / 2;
  constexpr int ROWS = CT_TF + KT - 1;
  constexpr int FC = 16;
  __shared__ __attribute__((aligned(16))) float g[ROWS][CT_CW];
  __shared__ double red[4][2][CT_CW];
  const int tid = threadIdx.x;
  const int b = blockIdx.z, f0 = blockIdx.x * CT_TF, c0 = blockIdx.y * CT_CW;
  {
    const int q = tid & 7, ch8 = c0 + 8 * q;
    for (int r = tid >> 3; r < ROWS; r += 32) {
      const int f = f0 - P + r;
      f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
      if (f >= 0 && f < t && ch8 < c) {
        const size_t base = ((size_t)b * t + f) * 2 * c + ch8;
        const f32x4 a0 = *reinterpret_cast<const f32x4*>(u + base), a1 = *reinterpret_cast<const f32x4*>(u + base + 4);
        const f32x4 g0 = *reinterpret_cast<const f32x4*>(u + base + c), g1 = *reinterpret_cast<const f32x4*>(u + base + c + 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          lo[i] = a0[i] * sigmoid_ct(g0[i]);
          hi[i] = a1[i] * sigmoid_ct(g1[i]);
        }
      }
      *reinterpret_cast<f32x4*>(&g[r][8 * q]) = lo;
      *reinterpret_cast<f32x4*>(&g[r][8 * q + 4]) = hi;
    }
  }
  __syncthreads();
  const int lane = tid & 63, wv = tid >> 6;
  const int ch = c0 + lane, fs = f0 + wv * CT_FPT;
  const bool active = ch < c && fs < t;
  const int off = (KT - k) / 2;
  double s1 = 0.0, s2 = 0.0;
  if (active) {
    float w[KT <= 31 ? KT : 1];
    if constexpr (KT <= 31) {
#pragma unroll
      for (int j = 0; j < KT; ++j) w[j] = (j >= off && j < off + k) ? dw_w[(size_t)(j - off) * c + ch] : 0.f;
    }
#pragma unroll 1
    for (int f0c = 0; f0c < CT_FPT && fs + f0c < t; f0c += FC) {
      float acc[FC];
#pragma unroll
      for (int f = 0; f < FC; ++f) acc[f] = 0.f;
      const int r0 = wv * CT_FPT + f0c;
      if constexpr (KT <= 31) {
#pragma unroll
        for (int s = 0; s < FC + KT - 1; ++s) {
          const float v = g[r0 + s][lane];
#pragma unroll
          for (int f = 0; f < FC; ++f) {
            const int j = s - f;
            if (j >= 0 && j < KT) acc[f] = fmaf(w[j], v, acc[f]);
          }
        }
      } else {
        for (int j = 0; j < k; ++j) {
          const float wj = dw_w[(size_t)j * c + ch];
#pragma unroll
          for (int f = 0; f < FC; ++f) acc[f] = fmaf(wj, g[r0 + off + j + f][lane], acc[f]);
        }
      }
      const size_t zbase = ((size_t)b * t + fs + f0c) * c + ch;
#pragma unroll
      for (int f = 0; f < FC; ++f) {
        if (fs + f0c + f < t) {
          z[zbase + (size_t)f * c] = acc[f];
          const double d = (double)acc[f];
          s1 += d;
          s2 += d * d;
        }
      }
    }
  }
  red[wv][0][lane] = s1;
  red[wv][1][lane] = s2;
  __syncthreads();
  if (wv == 0 && ch < c) {
    const double a = (red[0][0][lane] + red[1][0][lane]) + (red[2][0][lane] + red[3][0][lane]);
    const double q = (red[0][1][lane] + red[1][1][lane]) + (red[2][1][lane] + red[3][1][lane]);
    const int cnt = t - f0 < CT_TF ? t - f0 : CT_TF;
    const double mean = a / cnt;
    const size_t wg = (size_t)b * gridDim.x + blockIdx.x;
    part[(wg * 3 + 0) * c + ch] = (double)cnt;
    part[(wg * 3 + 1) * c + ch] = mean;
    part[(wg * 3 + 2) * c + ch] = q - a * mean;          // float64: 50 standard deviations of mean cost 2500 x 2^-53 of the variance
  }
}

// one thread per channel: Chan's combine of the workgroups' (count, mean, M2) in float64, in workgroup order
__global__ __launch_bounds__(256) void ct_bn_stats_kernel(const double* __restrict__ part, int n_parts, int c, float eps, float* __restrict__ mean_rstd,
                                                          float* __restrict__ mean_var) {
  const int ch = blockIdx.x * 256 + threadIdx.x;
  if (ch >= c) return;
  double n = 0.0, mean = 0.0, m2 = 0.0;
  for (int p = 0; p < n_parts; ++p) {
    const double nb = part[((size_t)p * 3 + 0) * c + ch], mb = part[((size_t)p * 3 + 1) * c + ch], qb = part[((size_t)p * 3 + 2) * c + ch];
    const double nn = n + nb, d = mb - mean;
    mean += d * (nb / nn);
    m2 += qb + d * d * (n * nb / nn);
    n = nn;
  }
  const double var = m2 / n;
  mean_rstd[ch] = (float)mean;
  mean_rstd[c + ch] = (float)(1.0 / sqrt(var + (double)eps));
  mean_var[ch] = (float)mean;
  mean_var[c + ch] = (float)var;
}

// ffn_act_cast_kernel (csrc/w2v_train.hip) with BatchNorm + activation in place of bias + GELU + dropout: 64 x 64 tiles, a thread owns four
// consecutive channels of four rows, the transposed copy leaves through LDS as 4-byte stores of two consecutive rows
__global__ __launch_bounds__(256) void ct_bn_act_cast_kernel(const float* __restrict__ z, const float* __restrict__ mean_rstd, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, int rows, int c, int act, unsigned short* __restrict__ y,
                                                             unsigned short* __restrict__ yt, long long ldt, int rows_pad) {
  __shared__ unsigned short tile[64][66];
  const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
  const int tx4 = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int cc = c0 + 4 * tx4;
  f32x4 mu = {0.f, 0.f, 0.f, 0.f}, sc = mu, bt = mu;
  if (cc < c) {
    mu = *reinterpret_cast<const f32x4*>(mean_rstd + cc);
    sc = *reinterpret_cast<const f32x4*>(mean_rstd + c + cc) * *reinterpret_cast<const f32x4*>(gamma + cc);
    bt = *reinterpret_cast<const f32x4*>(beta + cc);
  }
#pragma unroll
  for (int pass = 0; pass < 4; ++pass) {
    const int i = ty + 16 * pass, r = r0 + i;
    unsigned lo = 0, hi = 0;
    if (r < rows && cc < c) {
      f32x4 v = *reinterpret_cast<const f32x4*>(z + (size_t)r * c + cc);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = act_ct(fmaf(v[e] - mu[e], sc[e], bt[e]), act);
      lo = pack_bf16(v[0], v[1]); hi = pack_bf16(v[2], v[3]);
      if (y) *reinterpret_cast<u32x2*>(y + (size_t)r * c + cc) = u32x2{lo, hi};
    }
    tile[i][4 * tx4 + 0] = (unsigned short)(lo & 0xffffu); tile[i][4 * tx4 + 1] = (unsigned short)(lo >> 16);
    tile[i][4 * tx4 + 2] = (unsigned short)(hi & 0xffffu); tile[i][4 * tx4 + 3] = (unsigned short)(hi >> 16);
  }
  __syncthreads();
  if (yt) {
    const int tp = threadIdx.x & 31, tg = threadIdx.x >> 5;
    for (int i = tg; i < 64; i += 8) {
      const int col = c0 + i, r = r0 + 2 * tp;
      if (col < c && r + 1 < rows_pad) *reinterpret_cast<unsigned*>(yt + (size_t)col * ldt + r) = (unsigned)tile[2 * tp][i] | ((unsigned)tile[2 * tp + 1][i] << 16);
      else if (col < c && r < rows_pad) yt[(size_t)col * ldt + r] = tile[2 * tp][i];
    }
  }
}

// d gamma / d beta partials: workgroup = (64 channels, CT_SR = 32 rows), lane = channel, wave w the rows w, w + 4, ... (eight per thread, all
// sixteen loads in flight: with 128 rows per workgroup the launch had 512 workgroups of 32 dependent iterations and took 34.8 us at 3 992 x 1024,
// a ninth of the memory rate); the four waves' sums meet in LDS in wave order: part[row block][2][c] = (sum g zh, sum g)
__global__ __launch_bounds__(256) void ct_bn_act_bwd_sums_kernel(const float* __restrict__ z, const float* __restrict__ mean_rstd, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, const float* __restrict__ da, long long rows, int c, int act,
                                                                 float* __restrict__ part) {
  __shared__ float red[4][2][CT_CW];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int ch = blockIdx.x * CT_CW + lane;
  const long long r0 = (long long)blockIdx.y * CT_SR;
  float sg = 0.f, sgz = 0.f;
  if (ch < c) {
    const float mu = mean_rstd[ch], rs = mean_rstd[c + ch], gm = gamma[ch], bt = beta[ch];
#pragma unroll
    for (int i = 0; i < CT_SR / 4; ++i) {
      const long long r = r0 + wv + 4 * i;
      if (r < rows) {
        const float zh = (z[(size_t)r * c + ch] - mu) * rs;
        const float gg = da[(size_t)r * c + ch] * dact_ct(fmaf(gm, zh, bt), act);
        sg += gg;
        sgz = fmaf(gg, zh, sgz);
      }
    }
  }
  red[wv][0][lane] = sgz;
  red[wv][1][lane] = sg;
  __syncthreads();
  if (wv < 2 && ch < c)
    part[((size_t)blockIdx.y * 2 + wv) * c + ch] = (red[0][wv][lane] + red[1][wv][lane]) + (red[2][wv][lane] + red[3][wv][lane]);
}

// out[i] = sum_p part[p * stride + i] in float64 (the ordered finish of the partials above and of d dw_w): workgroup = 64 outputs, wave w sums the
// parts w, w + 4, ... in ascending order, the four sums meet in LDS in wave order.  Outputs i < n0 go to out0, the rest to out1 (d gamma | d beta
// from one launch).  One thread per output over all parts was a chain of n_parts dependent loads: 125 of them took longer than the partials.
__global__ __launch_bounds__(256) void ct_sum_parts_kernel(const float* __restrict__ part, long long n, int n_parts, long long stride, float* __restrict__ out0,
                                                           long long n0, float* __restrict__ out1) {
  __shared__ double red[4][CT_CW];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long i = (long long)blockIdx.x * CT_CW + lane;
  double a = 0.0;
  if (i < n) {
#pragma unroll 8
    for (int p = wv; p < n_parts; p += 4) a += (double)part[(size_t)p * stride + i];
  }
  red[wv][lane] = a;
  __syncthreads();
  if (wv == 0 && i < n) {
    const float r = (float)((red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]));
    if (i < n0) out0[i] = r;
    else out1[i - n0] = r;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// backward: activation, BatchNorm, depthwise conv, GLU
// ---------------------------------------------------------------------------------------------------------------------
// Workgroup = (128 frames, 64 channels, clip), as the forward.
//  1. stage dz for the frames f0 - P .. f0 + 127 + P (P = (KT - 1) / 2) in LDS [rows][64], lane = channel: zh and g recomputed from z and da,
//     dz = gamma rstd (g - dbeta / n - zh dgamma / n) (inv_n = 0 with running statistics); 0 outside [0, t).
//  2. lane l of wave w owns channel c0 + l and the frames f0 + 32 w .. + 31.  With the taps centred in KT and flipped (wf[j] = W[KT - 1 - j]) the
//     staged row r0 + f + j is dz[f - I + P] of tap I = KT - 1 - j, so ONE pass over a chunk's rows gives both
//        dG[f]   += wf[j] row      (the transposed conv)
//        dW[I]   += G[f] row       (the weight gradient; G[f] = GLU of the thread's own frame, recomputed)
//     KT <= 31: unrolled over (row, frame) with wf, dW and the chunk's dG in registers; 31 < k <= 63: a loop over the taps.
//  3. du from dG and the recomputed gate; the four waves' dW meet in LDS in wave order: part[wg][k][c].
template <int KT>
__global__ __launch_bounds__(256) void ct_glu_dwconv_bwd_kernel(const float* __restrict__ u, const float* __restrict__ z, const float* __restrict__ da, int t, int c,
                                                                const float* __restrict__ dw_w, int k, const float* __restrict__ mean_rstd,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                const float* __restrict__ dgamma, const float* __restrict__ dbeta, float inv_n, int act,
                                                                float* __restrict__ du, float* __restrict__ part) {
  constexpr int P = (KT - 1) / 2;
  constexpr int ROWS = CT_TF + KT - 1;
  constexpr int FC = KT <= 31 ? 16 : 32;
  constexpr bool REUSE = 4 * KT <= ROWS;              // the staged tile holds the four waves' dW once it has been read
  __shared__ __attribute__((aligned(16))) float g[ROWS][CT_CW];
  __shared__ float red_own[REUSE ? 1 : 4 * KT][CT_CW];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int b = blockIdx.z, f0 = blockIdx.x * CT_TF, c0 = blockIdx.y * CT_CW;
  const int ch = c0 + lane;
  const bool chok = ch < c;
  {
    float mu = 0.f, rs = 0.f, gm = 0.f, bt = 0.f, dbn = 0.f, dgn = 0.f;
    if (chok) {
      mu = mean_rstd[ch]; rs = mean_rstd[c + ch]; gm = gamma[ch]; bt = beta[ch];
      if (inv_n != 0.f) { dbn = dbeta[ch] * inv_n; dgn = dgamma[ch] * inv_n; }
    }
    const float gr = gm * rs;
#pragma unroll 8
    for (int r = wv; r < ROWS; r += 4) {
      const int f = f0 - P + r;
      float v = 0.f;
      if (chok && f >= 0 && f < t) {
        const size_t idx = ((size_t)b * t + f) * c + ch;
        const float zh = (z[idx] - mu) * rs;
        const float gg = da[idx] * dact_ct(fmaf(gm, zh, bt), act);
        v = gr * (gg - dbn - zh * dgn);
      }
      g[r][lane] = v;
    }
  }
  __syncthreads();
  const int fs = f0 + wv * CT_FPT;
  const bool active = chok && fs < t;
  const int off = (KT - k) / 2;
  float (*red)[CT_CW] = REUSE ? g : red_own;
  float dwacc[KT <= 31 ? KT : 1];
  if constexpr (KT <= 31) {
#pragma unroll
    for (int j = 0; j < KT; ++j) dwacc[j] = 0.f;
  }
  if (active) {
    float wf[KT <= 31 ? KT : 1];
    if constexpr (KT <= 31) {
#pragma unroll
      for (int j = 0; j < KT; ++j) {
        const int i = KT - 1 - j - off;              // the real tap behind flipped, centred position j
        wf[j] = (i >= 0 && i < k) ? dw_w[(size_t)i * c + ch] : 0.f;
      }
    }
#pragma unroll 1
    for (int f0c = 0; f0c < CT_FPT && fs + f0c < t; f0c += FC) {
      float acc[FC], gl[FC];
      const size_t ubase = ((size_t)b * t + fs + f0c) * 2 * c + ch;
#pragma unroll
      for (int f = 0; f < FC; ++f) {
        acc[f] = 0.f;
        gl[f] = 0.f;
        if (fs + f0c + f < t) gl[f] = u[ubase + (size_t)f * 2 * c] * sigmoid_ct(u[ubase + (size_t)f * 2 * c + c]);
      }
      const int r0 = wv * CT_FPT + f0c;
      if constexpr (KT <= 31) {
#pragma unroll
        for (int s = 0; s < FC + KT - 1; ++s) {
          const float v = g[r0 + s][lane];
#pragma unroll
          for (int f = 0; f < FC; ++f) {
            const int j = s - f;
            if (j >= 0 && j < KT) {
              acc[f] = fmaf(wf[j], v, acc[f]);
              dwacc[j] = fmaf(gl[f], v, dwacc[j]);
            }
          }
        }
      } else {
        for (int i = 0; i < k; ++i) {
          const int j = KT - 1 - i - off;
          const float wj = dw_w[(size_t)i * c + ch];
          float d = 0.f;
#pragma unroll
          for (int f = 0; f < FC; ++f) {
            const float v = g[r0 + f + j][lane];
            acc[f] = fmaf(wj, v, acc[f]);
            d = fmaf(gl[f], v, d);
          }
          red[wv * KT + j][lane] = d;                // FC = 32: the thread's whole run, one store per tap (its own slot of red_own)
        }
      }
#pragma unroll
      for (int f = 0; f < FC; ++f) {
        if (fs + f0c + f < t) {
          const float u1 = u[ubase + (size_t)f * 2 * c], s = sigmoid_ct(u[ubase + (size_t)f * 2 * c + c]);
          du[ubase + (size_t)f * 2 * c] = acc[f] * s;
          du[ubase + (size_t)f * 2 * c + c] = acc[f] * u1 * s * (1.f - s);
        }
      }
    }
  } else if constexpr (KT > 31) {
    for (int i = 0; i < k; ++i) red[wv * KT + (KT - 1 - i - off)][lane] = 0.f;
  }
  if constexpr (KT <= 31) {
    __syncthreads();                                  // every wave has read its staged rows: the tile becomes the waves' dW
#pragma unroll
    for (int j = 0; j < KT; ++j) red[wv * KT + j][lane] = dwacc[j];
  }
  __syncthreads();
  if (chok) {
    const size_t wg = (size_t)b * gridDim.x + blockIdx.x;
    for (int i = wv; i < k; i += 4) {
      const int j = KT - 1 - i - off;
      part[(wg * k + i) * c + ch] = (red[j][lane] + red[KT + j][lane]) + (red[2 * KT + j][lane] + red[3 * KT + j][lane]);
    }
  }
}

// dy = dy_v + R^T dy_rot, four channels per thread; the partner channel j ^ 32 of the same head is a second 16-byte load
__global__ __launch_bounds__(256) void ct_rotary_bwd_kernel(const float* __restrict__ dyv, const float* __restrict__ dyr, long long rows, int t, int c,
                                                            const float* __restrict__ cos_sin, int t_table, float* __restrict__ dy) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const int c4 = c >> 2;
  if (idx >= rows * c4) return;
  const long long row = idx / c4;
  const int i = (int)(idx - row * c4) * 4;
  const int pos = (int)(row % t);
  const f32x4 cv = *reinterpret_cast<const f32x4*>(cos_sin + (size_t)pos * 32 + (i & 31));
  const f32x4 sv = *reinterpret_cast<const f32x4*>(cos_sin + ((size_t)t_table + pos) * 32 + (i & 31));
  const f32x4 a = *reinterpret_cast<const f32x4*>(dyv + row * c + i);
  const f32x4 r = *reinterpret_cast<const f32x4*>(dyr + row * c + i);
  const f32x4 p = *reinterpret_cast<const f32x4*>(dyr + row * c + (i ^ 32));
  const float sgn = (i & 32) ? 1.f : -1.f;
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = a[e] + r[e] * cv[e] - sgn * p[e] * sv[e];
  *reinterpret_cast<f32x4*>(dy + row * c + i) = o;
}

// ffn_act_cast_kernel / ffn_act_bwd_kernel (csrc/w2v_train.hip) with SiLU
__global__ __launch_bounds__(256) void ct_ffn_silu_cast_kernel(const float* __restrict__ z, const float* __restrict__ bias, int rows, int c, float p, float scale,
                                                               unsigned long long seed, unsigned short* __restrict__ y, unsigned short* __restrict__ yt, long long ldt,
                                                               int rows_pad) {
  __shared__ unsigned short tile[64][66];
  const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
  const int tx4 = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
  for (int pass = 0; pass < 4; ++pass) {
    const int i = ty + 16 * pass, r = r0 + i, cc = c0 + 4 * tx4;
    unsigned lo = 0, hi = 0;
    if (r < rows && cc < c) {
      f32x4 v = *reinterpret_cast<const f32x4*>(z + (size_t)r * c + cc);
      if (bias) v += *reinterpret_cast<const f32x4*>(bias + cc);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = silu(v[e]);
      if (p > 0.f) {
        const Philox4 rn = philox(seed, PHILOX_DROPOUT, ((unsigned long long)r * c + cc) >> 2);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = u01(rn.v[e]) >= p ? v[e] * scale : 0.f;
      }
      lo = pack_bf16(v[0], v[1]); hi = pack_bf16(v[2], v[3]);
      if (y) *reinterpret_cast<u32x2*>(y + (size_t)r * c + cc) = u32x2{lo, hi};
    }
    tile[i][4 * tx4 + 0] = (unsigned short)(lo & 0xffffu); tile[i][4 * tx4 + 1] = (unsigned short)(lo >> 16);
    tile[i][4 * tx4 + 2] = (unsigned short)(hi & 0xffffu); tile[i][4 * tx4 + 3] = (unsigned short)(hi >> 16);
  }
  __syncthreads();
  if (yt) {
    const int tp = threadIdx.x & 31, tg = threadIdx.x >> 5;
    for (int i = tg; i < 64; i += 8) {
      const int col = c0 + i, r = r0 + 2 * tp;
      if (col < c && r + 1 < rows_pad) *reinterpret_cast<unsigned*>(yt + (size_t)col * ldt + r) = (unsigned)tile[2 * tp][i] | ((unsigned)tile[2 * tp + 1][i] << 16);
      else if (col < c && r < rows_pad) yt[(size_t)col * ldt + r] = tile[2 * tp][i];
    }
  }
}

__global__ __launch_bounds__(256) void ct_ffn_silu_bwd_kernel(const float* __restrict__ z, const float* __restrict__ bias, int c, const float* __restrict__ da, float p,
                                                              float scale, unsigned long long seed, float* __restrict__ dz, long long n4) {
  const long long i4 = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i4 >= n4) return;
  const long long e = i4 * 4;
  f32x4 v = *reinterpret_cast<const f32x4*>(z + e);
  if (bias) v += *reinterpret_cast<const f32x4*>(bias + (e % c));
  f32x4 gr = *reinterpret_cast<const f32x4*>(da + e);
  if (p > 0.f) {
    const Philox4 rn = philox(seed, PHILOX_DROPOUT, (unsigned long long)i4);
#pragma unroll
    for (int q = 0; q < 4; ++q) gr[q] = u01(rn.v[q]) >= p ? gr[q] * scale : 0.f;
  }
  f32x4 o;
#pragma unroll
  for (int q = 0; q < 4; ++q) o[q] = gr[q] * dact_ct(v[q], 2);
  *reinterpret_cast<f32x4*>(dz + e) = o;
}

inline bool bad_kernel(int kernel) { return kernel < 1 || kernel > 63 || !(kernel & 1); }
inline bool bad_act(int act) { return act != 1 && act != 2; }
inline long long tiles_of(int t) { return (t + CT_TF - 1) / CT_TF; }

}  // namespace
}  // namespace ts

using namespace ts;

extern "C" int ts_conformer_train_abi_version(void) { return TS_CONFORMER_TRAIN_ABI_VERSION; }

extern "C" int64_t ts_conformer_glu_dwconv_train_fwd_workspace(int32_t batch, int32_t t, int32_t c) {
  if (batch <= 0 || t <= 0 || c <= 0) return TS_EINVAL;
  return (int64_t)batch * tiles_of(t) * 3 * c * (int64_t)sizeof(double);
}

#define TS_CT_DISPATCH(KERNEL, ...)                                                                   \
  do {                                                                                                \
    if (kernel <= 3) hipLaunchKernelGGL((KERNEL<3>), grid, dim3(256), 0, stream, __VA_ARGS__);        \
    else if (kernel <= 7) hipLaunchKernelGGL((KERNEL<7>), grid, dim3(256), 0, stream, __VA_ARGS__);   \
    else if (kernel <= 15) hipLaunchKernelGGL((KERNEL<15>), grid, dim3(256), 0, stream, __VA_ARGS__); \
    else if (kernel <= 31) hipLaunchKernelGGL((KERNEL<31>), grid, dim3(256), 0, stream, __VA_ARGS__); \
    else hipLaunchKernelGGL((KERNEL<63>), grid, dim3(256), 0, stream, __VA_ARGS__);                   \
  } while (0)

extern "C" int ts_conformer_glu_dwconv_train_fwd(const float* u, int32_t batch, int32_t t, int32_t c, const float* dw_w, int32_t kernel, float* z,
                                                 void* workspace, void* stream_) {
  if (!u || !dw_w || !z || !workspace || batch <= 0 || t <= 0 || c <= 0) return TS_EINVAL;
  if (bad_kernel(kernel) || c % 8 || misaligned(u) || misaligned(dw_w) || misaligned(z) || misaligned(workspace) || batch > 65535) return TS_EUNSUPPORTED;
  TS_STREAM;
  const dim3 grid((unsigned)tiles_of(t), (unsigned)((c + CT_CW - 1) / CT_CW), (unsigned)batch);
  TS_CT_DISPATCH(ct_glu_dwconv_fwd_kernel, u, t, c, dw_w, kernel, z, static_cast<double*>(workspace));
  return hip_status(hipGetLastError());
}

extern "C" int ts_conformer_bn_stats(const void* workspace, int32_t batch, int32_t t, int32_t c, float eps, float* mean_rstd, float* mean_var, void* stream_) {
  if (!workspace || !mean_rstd || !mean_var || batch <= 0 || t <= 0 || c <= 0 || (long long)batch * t < 2) return TS_EINVAL;
  if (c % 8 || misaligned(workspace) || misaligned(mean_rstd) || misaligned(mean_var) || batch > 65535) return TS_EUNSUPPORTED;
  TS_STREAM;
  hipLaunchKernelGGL(ct_bn_stats_kernel, dim3(nblk(c)), dim3(256), 0, stream, static_cast<const double*>(workspace), (int)(batch * tiles_of(t)), c, eps,
                     mean_rstd, mean_var);
  return hip_status(hipGetLastError());
}

extern "C" int ts_conformer_bn_act_cast(const float* z, const float* mean_rstd, const float* gamma, const float* beta, int64_t rows, int32_t c, int32_t act,
                                        void* y, void* yt, int64_t ldt, int64_t rows_pad, void* stream_) {
  if (!z || !mean_rstd || !gamma || !beta || (!y && !yt) || rows <= 0 || c <= 0 || rows >= (1ll << 31)) return TS_EINVAL;
  if (yt && (rows_pad < rows || ldt < rows_pad || rows_pad >= (1ll << 31))) return TS_EINVAL;
  if (c % 8 || bad_act(act) || misaligned(z) || misaligned(mean_rstd) || misaligned(gamma) || misaligned(beta) || misaligned(y) ||
      (yt && (ldt % 2 || misaligned(yt))))
    return TS_EUNSUPPORTED;
  TS_STREAM;
  const long long rp = yt ? rows_pad : rows;
  hipLaunchKernelGGL(ct_bn_act_cast_kernel, dim3((unsigned)((c + 63) / 64), (unsigned)((rp + 63) / 64)), dim3(256), 0, stream, z, mean_rstd, gamma, beta,
                     (int)rows, (int)c, act, static_cast<unsigned short*>(y), static_cast<unsigned short*>(yt), (long long)ldt, (int)rows_pad);
  return hip_status(hipGetLastError());
}

extern "C" int64_t ts_conformer_bn_act_bwd_sums_workspace(int64_t rows, int32_t c) {
  if (rows <= 0 || c <= 0) return TS_EINVAL;
  return (rows + CT_SR - 1) / CT_SR * 2 * c * (int64_t)sizeof(float);
}

extern "C" int ts_conformer_bn_act_bwd_sums(const float* z, const float* mean_rstd, const float* gamma, const float* beta, const float* da, int64_t rows,
                                            int32_t c, int32_t act, float* dgamma, float* dbeta, void* workspace, void* stream_) {
  if (!z || !mean_rstd || !gamma || !beta || !da || !dgamma || !dbeta || !workspace || rows <= 0 || c <= 0 || rows >= (1ll << 31)) return TS_EINVAL;
  if (c % 8 || bad_act(act) || misaligned(z) || misaligned(mean_rstd) || misaligned(gamma) || misaligned(beta) || misaligned(da) || misaligned(dgamma) ||
      misaligned(dbeta) || misaligned(workspace) || (rows + CT_SR - 1) / CT_SR > 65535)
    return TS_EUNSUPPORTED;
  TS_STREAM;
  const int n_parts = (int)((rows + CT_SR - 1) / CT_SR);
  float* part = static_cast<float*>(workspace);
  hipLaunchKernelGGL(ct_bn_act_bwd_sums_kernel, dim3((unsigned)((c + CT_CW - 1) / CT_CW), (unsigned)n_parts), dim3(256), 0, stream, z, mean_rstd, gamma, beta,
                     da, (long long)rows, (int)c, act, part);
  hipLaunchKernelGGL(ct_sum_parts_kernel, dim3((unsigned)((2 * c + CT_CW - 1) / CT_CW)), dim3(256), 0, stream, part, (long long)2 * c, n_parts,
                     (long long)2 * c, dgamma, (long long)c, dbeta);
  return hip_status(hipGetLastError());
}

extern "C" int64_t ts_conformer_glu_dwconv_train_bwd_workspace(int32_t batch, int32_t t, int32_t c, int32_t kernel) {
  if (batch <= 0 || t <= 0 || c <= 0) return TS_EINVAL;
  if (bad_kernel(kernel)) return TS_EUNSUPPORTED;
  return (int64_t)batch * tiles_of(t) * kernel * c * (int64_t)sizeof(float);
}

extern "C" int ts_conformer_glu_dwconv_train_bwd(const float* u, const float* z, const float* da, int32_t batch, int32_t t, int32_t c, const float* dw_w,
                                                 int32_t kernel, const float* mean_rstd, const float* gamma, const float* beta, const float* dgamma,
                                                 const float* dbeta, int32_t running_stats, int32_t act, float* du, float* d_dw, void* workspace,
                                                 void* stream_) {
  if (!u || !z || !da || !dw_w || !mean_rstd || !gamma || !beta || !dgamma || !dbeta || !du || !d_dw || !workspace || batch <= 0 || t <= 0 || c <= 0)
    return TS_EINVAL;
  const long long n = (long long)batch * t;
  if (!running_stats && n < 2) return TS_EINVAL;
  if (bad_kernel(kernel) || c % 8 || bad_act(act) || batch > 65535 || misaligned(u) || misaligned(z) || misaligned(da) || misaligned(dw_w) ||
      misaligned(mean_rstd) || misaligned(gamma) || misaligned(beta) || misaligned(dgamma) || misaligned(dbeta) || misaligned(du) || misaligned(d_dw) ||
      misaligned(workspace))
    return TS_EUNSUPPORTED;
  TS_STREAM;
  const dim3 grid((unsigned)tiles_of(t), (unsigned)((c + CT_CW - 1) / CT_CW), (unsigned)batch);
  const float inv_n = running_stats ? 0.f : (float)(1.0 / (double)n);
  float* part = static_cast<float*>(workspace);
  TS_CT_DISPATCH(ct_glu_dwconv_bwd_kernel, u, z, da, t, c, dw_w, kernel, mean_rstd, gamma, beta, dgamma, dbeta, inv_n, act, du, part);
  const long long kc = (long long)kernel * c;
  hipLaunchKernelGGL(ct_sum_parts_kernel, dim3((unsigned)((kc + CT_CW - 1) / CT_CW)), dim3(256), 0, stream, part, kc, (int)(batch * tiles_of(t)), kc, d_dw,
                     kc, static_cast<float*>(nullptr));
  return hip_status(hipGetLastError());
}
#undef TS_CT_DISPATCH

extern "C" int ts_conformer_rotary_bwd(const float* dy_v, const float* dy_rot, int32_t batch, int32_t t, int32_t c, const float* cos_sin, int32_t t_table,
                                       float* dy, void* stream_) {
  if (!dy_v || !dy_rot || !cos_sin || !dy || batch <= 0 || t <= 0 || c <= 0 || t > t_table) return TS_EINVAL;
  if (c % 64 || misaligned(dy_v) || misaligned(dy_rot) || misaligned(cos_sin) || misaligned(dy) || batch > 65535) return TS_EUNSUPPORTED;
  TS_STREAM;
  const long long rows = (long long)batch * t;
  hipLaunchKernelGGL(ct_rotary_bwd_kernel, dim3(nblk(rows * (c / 4))), dim3(256), 0, stream, dy_v, dy_rot, rows, t, c, cos_sin, t_table, dy);
  return hip_status(hipGetLastError());
}

extern "C" int ts_conformer_ffn_act_cast(const float* z, const float* bias, int64_t rows, int32_t c, int32_t act, float p_drop, uint64_t seed, void* y,
                                         void* yt, int64_t ldt, int64_t rows_pad, void* stream_) {
  if (act == 1) return ts_w2v_ffn_act_cast(z, bias, rows, c, p_drop, seed, y, yt, ldt, rows_pad, stream_);          // the same launch: the same bits
  if (!z || (!y && !yt) || rows <= 0 || c <= 0 || rows >= (1ll << 31) || !(p_drop >= 0.f && p_drop < 1.f)) return TS_EINVAL;
  if (yt && (rows_pad < rows || ldt < rows_pad || rows_pad >= (1ll << 31))) return TS_EINVAL;
  if (act != 2 || c % 4 || misaligned(z) || misaligned(bias) || misaligned(y, 7) || (yt && (ldt % 2 || misaligned(yt, 3)))) return TS_EUNSUPPORTED;
  TS_STREAM;
  const long long rp = yt ? rows_pad : rows;
  hipLaunchKernelGGL(ct_ffn_silu_cast_kernel, dim3((unsigned)((c + 63) / 64), (unsigned)((rp + 63) / 64)), dim3(256), 0, stream, z, bias, (int)rows, (int)c,
                     p_drop, 1.f / (1.f - p_drop), (unsigned long long)seed, static_cast<unsigned short*>(y), static_cast<unsigned short*>(yt), (long long)ldt,
                     (int)rows_pad);
  return hip_status(hipGetLastError());
}

extern "C" int ts_conformer_ffn_act_bwd(const float* z, const float* bias, int32_t c, int32_t act, const float* da, float p_drop, uint64_t seed, float* dz,
                                        int64_t n, void* stream_) {
  if (act == 1) return ts_w2v_ffn_act_bwd(z, bias, c, da, p_drop, seed, dz, n, stream_);
  if (!z || !da || !dz || n <= 0 || c <= 0 || n % c || !(p_drop >= 0.f && p_drop < 1.f)) return TS_EINVAL;
  if (act != 2 || c % 4 || misaligned(z) || misaligned(da) || misaligned(dz) || misaligned(bias)) return TS_EUNSUPPORTED;
  TS_STREAM;
  hipLaunchKernelGGL(ct_ffn_silu_bwd_kernel, dim3(nblk(n / 4)), dim3(256), 0, stream, z, bias, c, da, p_drop, 1.f / (1.f - p_drop), (unsigned long long)seed, dz,
                     (long long)(n / 4));
  return hip_status(hipGetLastError());
}
