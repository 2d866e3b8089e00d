// Training-mode encoder kernels, part 3 of 3 (csrc/train_dw.hip has the overview): the row-wise element kernels on the rows and element types
// of csrc/train_act.hpp -- time mask, residual add [+ ReLU] fwd / bwd (quartznet/blocks.py:332-337), import / export of the reference layout,
// the bf16 operand cast -- and the masked 1x1 convolution fwd / bwd-data / bwd-weight (MaskedConv1d with kernel_size = 1,
// quartznet/blocks.py:169-182).  The 1x1 convolution and its two backward products are plain GEMMs: the entry points here forward them to
// this library's own matrix-core GEMM (csrc/gemm_f32.hip; f32 or bf16 operands, f32 accumulation) -- no vendor library.  In bf16 the training
// step by default runs the forward and the data gradient on the inference kernel's pointwise-only mode (ts_tcs_subblock_fwd) and the weight
// gradient on csrc/train_gemm.hip (train_ops.set_pointwise_backend).
#include "ts_common.hpp"
#include "train_act.hpp"

namespace ts {

// y = x with frames >= len[b] zeroed (the re-masking in front of every MaskedConv1d, and of gradients on the way back)
template <class T>
__global__ __launch_bounds__(256) void mask_time_kernel(const T* __restrict__ x, const int* __restrict__ len, T* __restrict__ y,
                                                        int batch, int ch, int t, int pitch_x, int pitch_y) {
  TS_ROW_UNIT((long long)batch * ch);
  const int b = row / ch;
  // clamp_len written out, here and in add_rows: every caller in this file has t > i >= 0, and the compiler, which propagates argument ranges
  // into a helper from all its callers, would then compile these compares unsigned -- not the code these kernels had beside the depthwise ones
  int l = t;
  if (len) { l = len[b]; l = l < 0 ? 0 : (l > t ? t : l); }
  float v[8];
  load8(x + (size_t)row * pitch_x + i, v);
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = i + j < l ? v[j] : 0.f;
  store8(y + (size_t)row * pitch_y + i, v);
}

// out = relu(a + b) (RELU) or a + b; backward of the first: da = db = dout * (out > 0)
template <class T, bool RELU>
__device__ __forceinline__ void add_rows(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ o, long long rows, int t, int pitch,
                                         const int* __restrict__ len_b = nullptr, int ch = 1) {
  TS_ROW_UNIT(rows);
  const size_t base = (size_t)row * pitch + i;
  float x[8], z[8];
  load8(a + base, x);
  if (b) load8(b + base, z);
  if (len_b) {                                             // b counts only up to its clip's length (the mask of a MaskedConv1d input, backward)
    int l = len_b[row / ch];                               // clamp_len, written out (see mask_time_kernel)
    l = l < 0 ? 0 : (l > t ? t : l);
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = i + j < l ? z[j] : 0.f;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) { const float s = x[j] + (b ? z[j] : 0.f); x[j] = (!RELU || s > 0.f) ? s : 0.f; }
  store8(o + base, x);
}
template <class T>
__global__ __launch_bounds__(256) void add_relu_fwd_kernel(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ o, long long rows, int t, int pitch) {
  add_rows<T, true>(a, b, o, rows, t, pitch);
}
template <class T>
__global__ __launch_bounds__(256) void add_fwd_kernel(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ o, long long rows, int t, int pitch,
                                                      const int* __restrict__ len_b, int ch) {
  add_rows<T, false>(a, b, o, rows, t, pitch, len_b, ch);
}
template <class T>
__global__ __launch_bounds__(256) void relu_bwd_kernel(const T* __restrict__ dout, const T* __restrict__ out, T* __restrict__ din, long long rows, int t, int pitch) {
  TS_ROW_UNIT(rows);
  const size_t base = (size_t)row * pitch + i;
  float g[8], o[8];
  load8(dout + base, g);
  load8(out + base, o);
#pragma unroll
  for (int j = 0; j < 8; ++j) g[j] = o[j] > 0.f ? g[j] : 0.f;
  store8(din + base, g);
}

// sum of `parts` partial [rows] vectors (the per-clip dW of the pointwise backward)
__global__ __launch_bounds__(256) void sum_parts_kernel(const float* __restrict__ parts, float* __restrict__ out, long long rows, int n_parts) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows) return;
  float s = 0.f;
  for (int i = 0; i < n_parts; ++i) s += parts[(size_t)i * rows + idx];
  out[idx] = s;
}

// reference-layout f32 [rows][t] (contiguous) <-> pitched activation rows of either type: the boundary of the training path
template <class T>
__global__ __launch_bounds__(256) void act_import_kernel(const float* __restrict__ src, T* __restrict__ dst, long long rows, int t, int pitch) {
  TS_ROW_UNIT(rows);
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = i + j < t ? src[(size_t)row * t + i + j] : 0.f;
  store8(dst + (size_t)row * pitch + i, v);
}
template <class T>
__global__ __launch_bounds__(256) void act_export_kernel(const T* __restrict__ src, float* __restrict__ dst, long long rows, int t, int pitch) {
  TS_ROW_UNIT(rows);
  float v[8];
  load8(src + (size_t)row * pitch + i, v);
#pragma unroll
  for (int j = 0; j < 8; ++j) if (i + j < t) dst[(size_t)row * t + i + j] = v[j];
}

}  // namespace ts

using namespace ts;

extern "C" int ts_train_mask_time(const void* x, const int32_t* len, void* y, int32_t batch, int32_t ch, int32_t t, int32_t pitch_x,
                                  int32_t pitch_y, int32_t act, void* stream_) {
  if (!x || !len || !y || batch <= 0 || ch <= 0 || t <= 0 || act < 0 || act > 1) return TS_EINVAL;
  if (!rows_ok(x, pitch_x, act) || !rows_ok(y, pitch_y, act) || pitch_x < t || pitch_y < t) return TS_EINVAL;
  TS_STREAM;
  act_dispatch(act, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(mask_time_kernel<T>, row_grid((long long)batch * ch, t), dim3(256), 0, stream, as<T>(x), len, as<T>(y), batch, ch, t, pitch_x, pitch_y);
  });
  return hip_status(hipGetLastError());
}

extern "C" int ts_train_act_import(const float* src, void* dst, int64_t rows, int32_t t, int32_t pitch, int32_t act, void* stream_) {
  if (!src || !dst || rows <= 0 || t <= 0 || pitch < t || act < 0 || act > 1 || !rows_ok(dst, pitch, act)) return TS_EINVAL;
  TS_STREAM;
  act_dispatch(act, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(act_import_kernel<T>, row_grid(rows, t), dim3(256), 0, stream, src, as<T>(dst), (long long)rows, t, pitch);
  });
  return hip_status(hipGetLastError());
}

extern "C" int ts_train_act_export(const void* src, float* dst, int64_t rows, int32_t t, int32_t pitch, int32_t act, void* stream_) {
  if (!src || !dst || rows <= 0 || t <= 0 || pitch < t || act < 0 || act > 1 || !rows_ok(src, pitch, act)) return TS_EINVAL;
  TS_STREAM;
  act_dispatch(act, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(act_export_kernel<T>, row_grid(rows, t), dim3(256), 0, stream, as<T>(src), dst, (long long)rows, t, pitch);
  });
  return hip_status(hipGetLastError());
}

// fp32 -> bf16 (round to nearest even): operand copies of the weights for the bf16 GEMMs
__global__ __launch_bounds__(256) void cast_bf16_kernel(const float* __restrict__ x, unsigned short* __restrict__ y, long long n) {
  const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i + 3 < n) {
    const float4 v = *reinterpret_cast<const float4*>(x + i);
    *reinterpret_cast<uint2*>(y + i) = uint2{pack_bf16(v.x, v.y), pack_bf16(v.z, v.w)};
  } else {
    for (long long j = i; j < n; ++j) y[j] = (unsigned short)(pack_bf16(x[j], 0.f) & 0xffffu);
  }
}

extern "C" int ts_train_cast_bf16(const float* x, void* y, int64_t n, void* stream_) {
  if (!x || !y || n <= 0) return TS_EINVAL;
  if (reinterpret_cast<uintptr_t>(x) % 16 || reinterpret_cast<uintptr_t>(y) % 8) return TS_EINVAL;
  TS_STREAM;
  hipLaunchKernelGGL(cast_bf16_kernel, dim3(blocks((n + 3) / 4)), dim3(256), 0, stream, x, static_cast<unsigned short*>(y), (long long)n);
  return hip_status(hipGetLastError());
}

// v[b] = W . u[b]   (W [c_out][c_in] row-major, u [B][c_in][pitch_u], v [B][c_out][pitch_v]); u is expected masked by the caller.
// precision 0: f32 operands and result; 1: u and w bf16, v f32 (the decoder's logits); 2: u, w and v bf16.  f32 accumulation always.
extern "C" int ts_train_pwconv_fwd(const void* u, const void* w, void* v, int32_t batch, int32_t c_in, int32_t c_out, int32_t t,
                                   int32_t pitch_u, int32_t pitch_v, int32_t precision, void* stream_) {
  if (!u || !w || !v || batch <= 0 || c_in <= 0 || c_out <= 0 || t <= 0 || pitch_u < t || pitch_v < t) return TS_EINVAL;
  if (precision < 0 || precision > 2) return TS_EUNSUPPORTED;
  TS_STREAM;
  // per clip: V[c_out][t] = W[c_out][c_in] . U[c_in][t]  (W's contraction index contiguous, U's frame index contiguous)
  return gemm_f32(stream, precision != 0, w, c_in, 1, 0, 0, u, pitch_u, 1, (long long)c_in * pitch_u, 0, v, pitch_v, (long long)c_out * pitch_v,
                  precision == 2, nullptr, c_out, t, c_in, 1, batch, false);
}

// du[b] = W^T . dv[b];  dW = sum_b dv[b] . u[b]^T  (workspace: batch * c_out * c_in floats, f32 always); precision as above
// (1: dv, u, w bf16 and du f32; 2: du bf16 as well)
extern "C" int ts_train_pwconv_bwd(const void* dv, const void* u, const void* w, void* du, float* dw, float* workspace, int32_t batch,
                                   int32_t c_in, int32_t c_out, int32_t t, int32_t pitch_u, int32_t pitch_v, int32_t precision, void* stream_) {
  if (!dv || !u || !w || !du || !dw || !workspace || batch <= 0 || c_in <= 0 || c_out <= 0 || t <= 0 || pitch_u < t || pitch_v < t) return TS_EINVAL;
  if (precision < 0 || precision > 2) return TS_EUNSUPPORTED;
  TS_STREAM;
  const bool bf = precision != 0;
  // per clip: dU[c_in][t] = W^T . dV[c_out][t]  (A(m, k) = W[k][m]: W's output index is the contiguous one here)
  if (int st = gemm_f32(stream, bf, w, 1, c_in, 0, 0, dv, pitch_v, 1, (long long)c_out * pitch_v, 0, du, pitch_u, (long long)c_in * pitch_u,
                        precision == 2, nullptr, c_in, t, c_out, 1, batch, false))
    return st;
  // per clip: dW_b[c_out][c_in] = dV[c_out][t] . U[c_in][t]^T (both contract over their contiguous frame index) -> workspace, summed below.
  // One partial per clip keeps every CU busy (16 tiles x 32 clips at 512 x 512); the pitch padding beyond t never enters (K = t).
  if (int st = gemm_f32(stream, bf, dv, pitch_v, 1, (long long)c_out * pitch_v, 0, u, 1, pitch_u, (long long)c_in * pitch_u, 0, workspace, c_in,
                        (long long)c_in * c_out, false, nullptr, c_out, c_in, t, 1, batch, false))
    return st;
  const long long rows = (long long)c_in * c_out;
  hipLaunchKernelGGL(sum_parts_kernel, dim3(blocks(rows)), dim3(256), 0, stream, workspace, dw, rows, batch);
  return hip_status(hipGetLastError());
}

extern "C" int ts_train_add_relu_fwd(const void* a, const void* b, void* out, int64_t rows, int32_t t, int32_t pitch, int32_t act, void* stream_) {
  if (!a || !out || rows <= 0 || t <= 0 || pitch < t || act < 0 || act > 1) return TS_EINVAL;
  if (!rows_ok(a, pitch, act) || !rows_ok(out, pitch, act) || (b && !rows_ok(b, pitch, act))) return TS_EINVAL;
  TS_STREAM;
  act_dispatch(act, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(add_relu_fwd_kernel<T>, row_grid(rows, t), dim3(256), 0, stream, as<T>(a), as<T>(b), as<T>(out), (long long)rows, t, pitch);
  });
  return hip_status(hipGetLastError());
}

extern "C" int ts_train_add(const void* a, const void* b, const int32_t* len_b, int32_t ch, void* out, int64_t rows, int32_t t, int32_t pitch,
                            int32_t act, void* stream_) {
  if (!a || !b || !out || rows <= 0 || t <= 0 || pitch < t || act < 0 || act > 1 || (len_b && (ch <= 0 || rows % ch))) return TS_EINVAL;
  if (!rows_ok(a, pitch, act) || !rows_ok(out, pitch, act) || !rows_ok(b, pitch, act)) return TS_EINVAL;
  TS_STREAM;
  act_dispatch(act, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(add_fwd_kernel<T>, row_grid(rows, t), dim3(256), 0, stream, as<T>(a), as<T>(b), as<T>(out), (long long)rows, t, pitch, len_b, ch);
  });
  return hip_status(hipGetLastError());
}

extern "C" int ts_train_relu_bwd(const void* dout, const void* out, void* din, int64_t rows, int32_t t, int32_t pitch, int32_t act, void* stream_) {
  if (!dout || !out || !din || rows <= 0 || t <= 0 || pitch < t || act < 0 || act > 1) return TS_EINVAL;
  if (!rows_ok(dout, pitch, act) || !rows_ok(out, pitch, act) || !rows_ok(din, pitch, act)) return TS_EINVAL;
  TS_STREAM;
  act_dispatch(act, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(relu_bwd_kernel<T>, row_grid(rows, t), dim3(256), 0, stream, as<T>(dout), as<T>(out), as<T>(din), (long long)rows, t, pitch);
  });
  return hip_status(hipGetLastError());
}
