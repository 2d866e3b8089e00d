// The row-wise kernels of the wav2vec2 encoder (inference), time-major fp32 [rows][C]:
//   ts_w2v_layernorm_fwd  y = [gelu] LN(x (+ xbias) (+ res)), f32 result and / or the bf16 copy the next product reads
//   ts_w2v_mask_rows      rows >= len[b] of every clip become 0
//   ts_w2v_glu_fwd        y = x[:, :c] * sigmoid(x[:, c:]): the activation of the adapter layers behind the encoder (config.add_adapter)
// conformer_ln_rotary_kernel (csrc/conformer.hip) and ln_bwd_kernel (csrc/w2v_train.hip) hold a row the way w2v_layernorm_kernel does; why the three
// do not share the code: csrc/w2v_rows.hpp.
#include "w2v_rows.hpp"

namespace ts {

// one wavefront per row: y = LN(x (+ xbias) (+ res)) * w + b.  NV float4 per lane hold the row (c <= 256 NV, c % 4 == 0):
// one read of the inputs, fp32 statistics in registers (mean, then centred sum of squares), one write of each output.
template <int NV>
__global__ __launch_bounds__(256) void w2v_layernorm_kernel(const float* __restrict__ x, const float* __restrict__ res,
                                                            const float* __restrict__ xbias, const float* __restrict__ w,
                                                            const float* __restrict__ b, float* __restrict__ y, long long rows, int c,
                                                            float eps, unsigned short* __restrict__ y16, int act) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* xr = x + row * c;
  const float* rr = res ? res + row * c : nullptr;
  float4 v[NV];
  float s = 0.f;
#pragma unroll
  for (int it = 0; it < NV; ++it) {
    const int i = (it * 64 + lane) * 4;
    v[it] = float4{0.f, 0.f, 0.f, 0.f};
    if (i < c) {
      v[it] = *reinterpret_cast<const float4*>(xr + i);
      if (rr) { const float4 r4 = *reinterpret_cast<const float4*>(rr + i); v[it].x += r4.x; v[it].y += r4.y; v[it].z += r4.z; v[it].w += r4.w; }
      if (xbias) { const float4 b4 = *reinterpret_cast<const float4*>(xbias + i); v[it].x += b4.x; v[it].y += b4.y; v[it].z += b4.z; v[it].w += b4.w; }
      s += (v[it].x + v[it].y) + (v[it].z + v[it].w);
    }
  }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);        // written out (as the q loop): wave_sum here changes the kernel's register moves
  const float mu = s / c;
  float q = 0.f;
#pragma unroll
  for (int it = 0; it < NV; ++it) {
    const int i = (it * 64 + lane) * 4;
    if (i < c) {
      const float d0 = v[it].x - mu, d1 = v[it].y - mu, d2 = v[it].z - mu, d3 = v[it].w - mu;
      q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    }
  }
  for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
  const float rs = rsqrtf(q / c + eps);
#pragma unroll
  for (int it = 0; it < NV; ++it) {
    const int i = (it * 64 + lane) * 4;
    if (i < c) {
      const float4 w4 = *reinterpret_cast<const float4*>(w + i), b4 = *reinterpret_cast<const float4*>(b + i);
      float4 o4 = float4{(v[it].x - mu) * rs * w4.x + b4.x, (v[it].y - mu) * rs * w4.y + b4.y, (v[it].z - mu) * rs * w4.z + b4.z,
                         (v[it].w - mu) * rs * w4.w + b4.w};
      if (act) o4 = float4{gelu_erf(o4.x), gelu_erf(o4.y), gelu_erf(o4.z), gelu_erf(o4.w)};
      if (y) *reinterpret_cast<float4*>(y + row * c + i) = o4;
      if (y16) *reinterpret_cast<uint2*>(y16 + row * c + i) = uint2{pack_bf16(o4.x, o4.y), pack_bf16(o4.z, o4.w)};
    }
  }
}

// rows >= len[b] of a [B][T][C] tensor become 0 (hidden_states[~attention_mask] = 0)
__global__ __launch_bounds__(256) void w2v_mask_rows_kernel(float* __restrict__ x, const int* __restrict__ len, int t, int c) {
  const int b = blockIdx.y;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const int n = len[b] < 0 ? 0 : (len[b] < t ? len[b] : t);      // key_limit clamps in the other order: other scalar compares
  const long long total = (long long)(t - n) * c;
  if (idx < total) x[((size_t)b * t + n) * c + idx] = 0.f;
}

// GLU over the channel halves of a row: y[r][j] = x[r][j] * sigmoid(x[r][c + j]) -- the activation of Wav2Vec2AdapterLayer (Conv1d to 2c channels, then
// nn.functional.glu over them); four channels per thread, f32 result and optional bf16 copy
__global__ __launch_bounds__(256) void w2v_glu_kernel(const float* __restrict__ x, float* __restrict__ y, unsigned short* __restrict__ y16, long long rows, int c) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const int q = c >> 2;
  if (idx >= rows * q) return;
  const long long r = idx / q;
  const int j = (int)(idx - r * q) * 4;
  const f32x4 a = *reinterpret_cast<const f32x4*>(x + r * 2 * c + j);
  const f32x4 g = *reinterpret_cast<const f32x4*>(x + r * 2 * c + c + j);
  f32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = a[i] / (1.f + __expf(-g[i]));
  *reinterpret_cast<f32x4*>(y + r * c + j) = o;
  if (y16) *reinterpret_cast<u32x2*>(y16 + r * c + j) = u32x2{pack_bf16(o[0], o[1]), pack_bf16(o[2], o[3])};
}

}  // namespace ts

using namespace ts;

extern "C" int ts_w2v_layernorm_fwd(const float* x, const float* res, const float* xbias, const float* w, const float* b, float eps,
                                    int64_t rows, int32_t c, int32_t act, float* y, void* y_bf16, void* stream_) {
  if (!x || !w || !b || (!y && !y_bf16) || rows <= 0 || c <= 0) return TS_EINVAL;
  if (c % 4 || c > 4096) return TS_EUNSUPPORTED;
  // the kernel moves float4s (8-byte pairs for the bf16 copy): as in ts_w2v_layernorm_bwd, a misaligned pointer is refused before any launch
  if (misaligned(x) || misaligned(res) || misaligned(xbias) || misaligned(w) || misaligned(b) || misaligned(y) || misaligned(y_bf16, 7)) return TS_EUNSUPPORTED;
  TS_STREAM;
  const dim3 grid((unsigned)((rows + 3) / 4));
  unsigned short* y16 = static_cast<unsigned short*>(y_bf16);
#define TS_LN(NV_) hipLaunchKernelGGL(w2v_layernorm_kernel<NV_>, grid, dim3(256), 0, stream, x, res, xbias, w, b, y, (long long)rows, c, eps, y16, act)
  if (c <= 512) TS_LN(2); else if (c <= 1024) TS_LN(4); else if (c <= 2048) TS_LN(8); else TS_LN(16);
#undef TS_LN
  return hip_status(hipGetLastError());
}

extern "C" int ts_w2v_mask_rows(float* x, int32_t batch, int32_t t, int32_t c, const int32_t* len, void* stream_) {
  if (!x || !len || batch <= 0 || t <= 0 || c <= 0) return TS_EINVAL;
  TS_STREAM;
  hipLaunchKernelGGL(w2v_mask_rows_kernel, dim3(nblk((long long)t * c), batch), dim3(256), 0, stream, x, len, t, c);
  return hip_status(hipGetLastError());
}

extern "C" int ts_w2v_glu_fwd(const float* x, int64_t rows, int32_t c, float* y, void* y_bf16, void* stream_) {
  if (!x || !y || rows <= 0 || c <= 0) return TS_EINVAL;
  if (c % 4 || misaligned(x) || misaligned(y) || misaligned(y_bf16, 7)) return TS_EUNSUPPORTED;
  TS_STREAM;
  hipLaunchKernelGGL(w2v_glu_kernel, dim3(nblk(rows * (c / 4))), dim3(256), 0, stream, x, y, static_cast<unsigned short*>(y_bf16), (long long)rows, c);
  return hip_status(hipGetLastError());
}
