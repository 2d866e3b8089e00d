// The positional convolution of the wav2vec2 encoder, time-major fp32 [B][T][C]: a grouped conv over a zero-padded copy of the clip rows
// (kernel / 2 zero rows in front of each clip, [B][T + k][C]).  Inference and mixed-precision fine-tuning are in this one file because they share
// that padded-copy layout and, at 64 channels per group, the matrix-core kernel w2v_posconv_mfma_kernel.
//   ts_w2v_posconv_fwd     y = x + gelu(conv(x) + b): precision 1 with 64-channel groups on w2v_posconv_mfma_kernel; otherwise one batched GEMM
//                          per tap (csrc/gemm_f32.hip) over the padded copy and w2v_posconv_finish_kernel
//   ts_w2v_groupconv_fwd   y = conv(x) + b, same padding: a layer of data2vec-audio's stacked positional convs (per-tap GEMMs)
//   ts_w2v_posconv_train   fine-tuning forward (also saves the conv result z) and data gradient (the same product over the flipped taps)
//   ts_w2v_posconv_wgrad   fine-tuning weight gradient, w2v_posconv_wgrad_kernel
//   posconv_raw_conv       the conv alone (the kernel's raw-accumulator epilogue), behind ts_posconv_stack_conv of csrc/posconv_stack_train.hip
#include "w2v_rows.hpp"

namespace ts {

// ---------------------------------------------------------------------------------------------------------------------
// positional conv: zero-padded copy in, bias + GELU + residual out
// ---------------------------------------------------------------------------------------------------------------------
// xp: [B][T + k][C] with k/2 zero rows before and k - k/2 after each clip
template <typename T>
__global__ __launch_bounds__(256) void w2v_pad_rows_kernel(const float* __restrict__ x, T* __restrict__ xp, int t, int c, int k) {
  const int b = blockIdx.y;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = (long long)(t + k) * c;
  if (idx >= total) return;
  const long long r = idx / c;
  const int col = (int)(idx - r * c);
  const long long src = r - k / 2;
  const float v = (src >= 0 && src < t) ? x[((size_t)b * t + src) * c + col] : 0.f;
  if constexpr (sizeof(T) == 2) xp[(size_t)b * total + idx] = (T)(pack_bf16(v, 0.f) & 0xffffu);
  else xp[(size_t)b * total + idx] = v;
}

// PLAIN: y = conv + bias (a layer of Data2VecAudioPositionalConvEmbedding: its LayerNorm + GELU follow in ts_w2v_layernorm_fwd); else the wav2vec2 /
// hubert embedding y = x + gelu(conv + bias)
template <bool PLAIN>
__global__ __launch_bounds__(256) void w2v_posconv_finish_kernel(const float* __restrict__ x, const float* __restrict__ yp,
                                                                 const float* __restrict__ bias, float* __restrict__ y, int t,
                                                                 int c, int k) {
  const int b = blockIdx.y;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)t * c) return;
  const int col = (int)(idx % c);
  // conv output frame r of clip b was accumulated at padded row b (T + k) + r
  const float v = yp[(size_t)b * (t + k) * c + idx] + bias[col];
  y[(size_t)b * t * c + idx] = PLAIN ? v : x[(size_t)b * t * c + idx] + gelu_erf(v);
}

// ---------------------------------------------------------------------------------------------------------------------
// Positional conv as an implicit GEMM on the matrix cores (precision 1, 64 channels per group: wav2vec2-large).
//   workgroup = 128 frames x 64 output channels of one (clip, group); the 128 + k - 1 input rows it needs are staged ONCE in
//   LDS and tap j simply reads rows j .. j + 127 of that window (no im2col, no per-tap restaging);
//   waves 2 x 2: 64 frames x 32 channels each, v_mfma_f32_32x32x16_bf16, A = window rows (ds_read_b128), B = tap weights
//   [co][ci] straight from L2, prefetched one tap ahead.  Epilogue: + bias, GELU, + x (fp32 residual), coalesced along channels.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int PC_TT = 128;         // frames per workgroup
constexpr int PC_PITCH = 144;      // bytes per staged row (64 bf16 + 16)

struct PcArgs {
  const unsigned short* xp;        // [B][T + k][C] bf16, k/2 zero rows in front of each clip
  const unsigned short* w;         // [k][G][64 co][64 ci] bf16
  const float* bias;
  const float* x;                  // [B][T][C] fp32 (residual)
  float* y;
  int t, c, k, groups;
  float* z;                        // training (ts_w2v_posconv_train): the conv result before bias and GELU, or NULL
  int plain;                       // training, data gradient: y = x + conv (no bias, no GELU)
};

// RAW: the third epilogue, out = conv(src) -- the accumulator as it is, no bias, no GELU, no residual (ts_posconv_stack_conv: a layer of data2vec-audio's
// positional stack in training, whose bias + LayerNorm + GELU are a row kernel of csrc/posconv_stack_train.hip).  <false> is the kernel as it was.
template <bool RAW>
__global__ __launch_bounds__(256) void w2v_posconv_mfma_kernel(const PcArgs a) {
  extern __shared__ __attribute__((aligned(16))) char win[];                  // [PC_TT + k - 1][PC_PITCH]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, g = blockIdx.y, t0 = blockIdx.x * PC_TT;
  const int rows = PC_TT + a.k - 1;
  const int prow = a.t + a.k;
  const unsigned short* src = a.xp + ((size_t)b * prow + t0) * a.c + (size_t)g * 64;
  for (int chunk = tid; chunk < rows * 8; chunk += 256) {
    const int r = chunk >> 3, cc = chunk & 7;
    uint4 v = uint4{0u, 0u, 0u, 0u};
    if (t0 + r < prow) v = *reinterpret_cast<const uint4*>(src + (size_t)r * a.c + cc * 8);
    *reinterpret_cast<uint4*>(win + r * PC_PITCH + cc * 16) = v;
  }
  __syncthreads();
  const int wm = wave >> 1, wn = wave & 1;                                    // 64 frames x 32 channels per wave
  const int half = lane >> 5, n32 = lane & 31;
  f32x16 acc[2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[mt][i] = 0.f;
  const char* arow = win + (wm * 64 + n32) * PC_PITCH + half * 16;            // A: row = frame, 8 consecutive ci per k-step
  const uint4* wp = reinterpret_cast<const uint4*>(a.w + ((size_t)g * 64 + wn * 32 + n32) * 64 + 8 * half);
  const size_t tap_stride = (size_t)a.groups * 64 * 64 / 8;                   // uint4 units
  uint4 bf[4], bn[4], bnn[4];                    // weights of tap j, j + 1, j + 2: an L2 round trip is longer than one tap's MFMAs
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) bf[ks] = wp[2 * ks];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) bn[ks] = wp[(a.k > 1 ? tap_stride : 0) + 2 * ks];
  for (int j = 0; j < a.k; ++j) {
    if (j + 2 < a.k) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) bnn[ks] = wp[(size_t)(j + 2) * tap_stride + 2 * ks];
    }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        const s16x8 af = *reinterpret_cast<const s16x8*>(arow + (j + 32 * mt) * PC_PITCH + ks * 32);
        acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, __builtin_bit_cast(s16x8, bf[ks]), acc[mt], 0, 0, 0);
      }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) { bf[ks] = bn[ks]; bn[ks] = bnn[ks]; }
  }
  const int co = g * 64 + wn * 32 + n32;
  const float bv = a.bias ? a.bias[co] : 0.f;
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int t = t0 + wm * 64 + 32 * mt + 8 * (i >> 2) + 4 * half + (i & 3);
      if (t < a.t) {
        const size_t o = ((size_t)b * a.t + t) * a.c + co;
        if constexpr (RAW) a.y[o] = acc[mt][i];
        else if (a.plain) a.y[o] = a.x[o] + acc[mt][i];
        else {
          if (a.z) a.z[o] = acc[mt][i];
          a.y[o] = a.x[o] + gelu_erf(acc[mt][i] + bv);
        }
      }
    }
}

// bf16 copy of x [B][t][c] f32 with `front` zero rows before and prow - front - t after each clip (prow rows per clip), one row of zeros behind the last clip
__global__ __launch_bounds__(256) void posconv_pad16_kernel(const float* __restrict__ x, unsigned short* __restrict__ xp, int t, int c, int prow, int front, long long total) {
  const long long idx = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (idx >= total) return;
  const long long row = idx / c;
  const int col = (int)(idx - row * c);
  const long long b = row / prow;
  const int r = (int)(row - b * prow) - front;
  f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
  if (r >= 0 && r < t && b * prow < total / c - 1) v = *reinterpret_cast<const f32x4*>(x + ((size_t)b * t + r) * c + col);
  *reinterpret_cast<u32x2*>(xp + idx) = u32x2{pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3])};
}

// Weight gradient of the positional conv on the matrix cores (mixed-precision fine-tuning):
//   dW[j][g][o][i] = sum_b sum_t dz[b][t][64 g + o] xp[b][t + j][64 g + i],   xp = x behind kernel / 2 zero rows per clip (the forward's padded copy)
// -- for one (group, tap) a 64 x 64 product contracted over all B T frames; the f32 GEMM of round 5 needed 2.6 ms for the 2 048 of them.  Workgroup =
// (8 taps, group), four waves of two taps each; a stage is 128 frames of one clip: the dz tile [128][64] and the xp window [128 + 8][64] (shared by the
// eight taps) in LDS as bf16, both operands out of them with transposing reads (rows = the contraction index t), v_mfma_f32_32x32x16_bf16, 128 f32
// accumulators per lane; the next stage's rows travel global -> registers while the current one is multiplied.  256 workgroups, each owning its
// outputs: no partials, no atomics.
constexpr int PW_TT = 128, PW_TAPS = 8, PW_WIN = PW_TT + PW_TAPS;
struct PwArgs {
  const unsigned short* dz;        // [B][T][C] bf16
  const unsigned short* xp;        // [B][T + k][C] bf16
  float* dw;                       // [k][G][64][64]
  int batch, t, c, k, groups;
};
__global__ __launch_bounds__(256) void w2v_posconv_wgrad_kernel(const PwArgs a) {
  __shared__ __attribute__((aligned(16))) char dzs[PW_TT * PC_PITCH];
  __shared__ __attribute__((aligned(16))) char xps[PW_WIN * PC_PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j0 = blockIdx.x * PW_TAPS, g = blockIdx.y;
  const int prow = a.t + a.k, n_ch = (a.t + PW_TT - 1) / PW_TT, S = a.batch * n_ch;
  f32x16 acc[2][2][2];
#pragma unroll
  for (int tp = 0; tp < 2; ++tp)
#pragma unroll
    for (int mo = 0; mo < 2; ++mo)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[tp][mo][ni][r] = 0.f;
  // staging: 16-byte chunks; the dz tile is 128 x 8 chunks = 4 per thread, the xp window 136 x 8 = 1 088 chunks = 4.25 per thread
  uint4 rz[4], rx[5];
  auto fetch = [&](int s) {
    const int b = s / n_ch, t0 = (s % n_ch) * PW_TT;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int chunk = tid + 256 * q, r = chunk >> 3, cc = chunk & 7;
      rz[q] = (t0 + r < a.t) ? *reinterpret_cast<const uint4*>(a.dz + ((size_t)b * a.t + t0 + r) * a.c + (size_t)g * 64 + cc * 8) : uint4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      const int chunk = tid + 256 * q, r = chunk >> 3, cc = chunk & 7;
      const int row = t0 + j0 + r;                        // row of the clip's padded copy
      rx[q] = (chunk < PW_WIN * 8 && row < prow) ? *reinterpret_cast<const uint4*>(a.xp + ((size_t)b * prow + row) * a.c + (size_t)g * 64 + cc * 8) : uint4{0u, 0u, 0u, 0u};
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int q = 0; q < 4; ++q) { const int chunk = tid + 256 * q; *reinterpret_cast<uint4*>(dzs + (chunk >> 3) * PC_PITCH + (chunk & 7) * 16) = rz[q]; }
#pragma unroll
    for (int q = 0; q < 5; ++q) { const int chunk = tid + 256 * q; if (chunk < PW_WIN * 8) *reinterpret_cast<uint4*>(xps + (chunk >> 3) * PC_PITCH + (chunk & 7) * 16) = rx[q]; }
  };
  const int half = lane >> 5, q4 = (lane >> 2) & 3, gq = (lane >> 4) & 1, p4 = lane & 3;
  const int tr_off = (8 * half + q4) * PC_PITCH + (16 * gq + 4 * p4) * 2;        // transposing read: rows = contraction index, columns = M / N index
  auto tr8 = [&](const char* p) {
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((TS_LDS s16x4*)((TS_LDS char*)p));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((TS_LDS s16x4*)((TS_LDS char*)p + 4 * PC_PITCH));
    return s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  };
  if (S > 0) fetch(0);
  for (int s = 0; s < S; ++s) {
    __syncthreads();                                       // the previous stage has been multiplied
    stage();
    __syncthreads();
    if (s + 1 < S) fetch(s + 1);
#pragma unroll
    for (int ks = 0; ks < PW_TT / 16; ++ks) {
      s16x8 af[2], bf[2][2];
#pragma unroll
      for (int mo = 0; mo < 2; ++mo) af[mo] = tr8(dzs + 16 * ks * PC_PITCH + tr_off + 64 * mo);
#pragma unroll
      for (int tp = 0; tp < 2; ++tp)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) bf[tp][ni] = tr8(xps + (16 * ks + 2 * wave + tp) * PC_PITCH + tr_off + 64 * ni);
#pragma unroll
      for (int tp = 0; tp < 2; ++tp)
#pragma unroll
        for (int mo = 0; mo < 2; ++mo)
#pragma unroll
          for (int ni = 0; ni < 2; ++ni) acc[tp][mo][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[mo], bf[tp][ni], acc[tp][mo][ni], 0, 0, 0);
    }
  }
  // accumulator register r of block (mo, ni): o = 32 mo + (r & 3) + 8 (r >> 2) + 4 half, i = 32 ni + lane % 32
#pragma unroll
  for (int tp = 0; tp < 2; ++tp) {
    const int j = j0 + 2 * wave + tp;
    if (j >= a.k) continue;
    float* const out = a.dw + ((size_t)j * a.groups + g) * 64 * 64;
#pragma unroll
    for (int mo = 0; mo < 2; ++mo)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r) out[(size_t)(32 * mo + (r & 3) + 8 * (r >> 2) + 4 * half) * 64 + 32 * ni + (lane & 31)] = acc[tp][mo][ni][r];
  }
}

}  // namespace ts

using namespace ts;

// out = conv(src) on w2v_posconv_mfma_kernel<true>; the arguments were checked by ts_posconv_stack_conv (csrc/posconv_stack_train.hip), its only caller.
// `front` zero rows in front of each clip in the padded bf16 copy (workspace: ts_w2v_posconv_train_workspace bytes).
int ts::posconv_raw_conv(hipStream_t stream, const float* src, int batch, int t, int c, const void* w_taps_bf16, int kernel, int groups, int front, float* out,
                         void* workspace) {
  const int prow = t + kernel;
  unsigned short* const xp = static_cast<unsigned short*>(workspace);
  const long long total = ((long long)batch * prow + 1) * c;
  hipLaunchKernelGGL(posconv_pad16_kernel, dim3(nblk(total / 4)), dim3(256), 0, stream, src, xp, t, c, prow, front, total);
  PcArgs pa{};
  pa.xp = xp; pa.w = static_cast<const unsigned short*>(w_taps_bf16); pa.y = out;
  pa.t = t; pa.c = c; pa.k = kernel; pa.groups = groups;
  hipLaunchKernelGGL(w2v_posconv_mfma_kernel<true>, dim3((t + PC_TT - 1) / PC_TT, groups, batch), dim3(256), (size_t)(PC_TT + kernel - 1) * PC_PITCH, stream, pa);
  return hip_status(hipGetLastError());
}

extern "C" int64_t ts_w2v_posconv_workspace_bytes(int32_t batch, int32_t t, int32_t c, int32_t kernel) {
  if (batch <= 0 || t <= 0 || c <= 0 || kernel <= 0) return TS_EINVAL;
  return (int64_t)2 * batch * (t + kernel) * c * sizeof(float);
}

static int posconv_impl(const float* x, int32_t batch, int32_t t, int32_t c, const void* w_taps, const float* bias, int32_t kernel,
                            int32_t groups, int32_t precision, float* y, void* workspace, void* stream_, bool plain) {
  if (!x || !w_taps || !bias || !y || !workspace || batch <= 0 || t <= 0 || c <= 0 || kernel <= 0 || groups <= 0 || c % groups) return TS_EINVAL;
  if (precision < 0 || precision > 1) return TS_EUNSUPPORTED;
  TS_STREAM;
  const int cg = c / groups;
  const long long prow = (long long)t + kernel;                       // padded rows per clip
  // workspace: yp f32 [B (t+k)][c] first, then the padded copy (f32 or bf16)
  float* yp = static_cast<float*>(workspace);
  char* xp = reinterpret_cast<char*>(yp + (size_t)batch * prow * c);
  const size_t es = precision ? 2 : 4;
  if (precision) hipLaunchKernelGGL(w2v_pad_rows_kernel<unsigned short>, dim3(nblk(prow * c), batch), dim3(256), 0, stream, x,
                                    reinterpret_cast<unsigned short*>(xp), t, c, kernel);
  else hipLaunchKernelGGL(w2v_pad_rows_kernel<float>, dim3(nblk(prow * c), batch), dim3(256), 0, stream, x, reinterpret_cast<float*>(xp), t, c, kernel);
  const size_t win_lds = (size_t)(PC_TT + kernel - 1) * PC_PITCH;
  if (!plain && precision && cg == 64 && win_lds <= 64 * 1024) {           // the fused kernel's epilogue is the wav2vec2 one
    PcArgs pa{};
    pa.xp = reinterpret_cast<const unsigned short*>(xp); pa.w = static_cast<const unsigned short*>(w_taps); pa.bias = bias; pa.x = x; pa.y = y;
    pa.t = t; pa.c = c; pa.k = kernel; pa.groups = groups;
    hipLaunchKernelGGL(w2v_posconv_mfma_kernel<false>, dim3((t + PC_TT - 1) / PC_TT, groups, batch), dim3(256), win_lds, stream, pa);
    return hip_status(hipGetLastError());
  }
  // all clips at once: output row r (over the padded row space) = sum_j xp[r + j] W_j^T, per group; rows between clips are waste
  const long long m = (long long)batch * prow - kernel;
  for (int j = 0; j < kernel; ++j) {
    if (int st = gemm_nt(stream, precision != 0, m, cg, cg, xp + (size_t)j * c * es, c, cg,
                         static_cast<const char*>(w_taps) + (size_t)j * groups * cg * cg * es, cg, (long long)cg * cg, yp, c, cg,
                         j ? 1.f : 0.f, groups))
      return st;
  }
  if (plain) hipLaunchKernelGGL(w2v_posconv_finish_kernel<true>, dim3(nblk((long long)t * c), batch), dim3(256), 0, stream, x, yp, bias, y, t, c, kernel);
  else hipLaunchKernelGGL(w2v_posconv_finish_kernel<false>, dim3(nblk((long long)t * c), batch), dim3(256), 0, stream, x, yp, bias, y, t, c, kernel);
  return hip_status(hipGetLastError());
}

extern "C" int ts_w2v_posconv_fwd(const float* x, int32_t batch, int32_t t, int32_t c, const void* w_taps, const float* bias,
                                  int32_t kernel, int32_t groups, int32_t precision, float* y, void* y_bf16, void* workspace,
                                  void* stream_) {
  (void)y_bf16;
  return posconv_impl(x, batch, t, c, w_taps, bias, kernel, groups, precision, y, workspace, stream_, false);
}

extern "C" int ts_w2v_groupconv_fwd(const float* x, int32_t batch, int32_t t, int32_t c, const void* w_taps, const float* bias,
                                    int32_t kernel, int32_t groups, int32_t precision, float* y, void* workspace, void* stream_) {
  return posconv_impl(x, batch, t, c, w_taps, bias, kernel, groups, precision, y, workspace, stream_, true);
}

extern "C" int64_t ts_w2v_posconv_wgrad_workspace(int32_t batch, int32_t t, int32_t c, int32_t kernel) {
  if (batch <= 0 || t <= 0 || c <= 0 || kernel <= 0) return TS_EINVAL;
  return (((int64_t)batch * (t + kernel) + 1) * c * 2 + 15) / 16 * 16 + ((int64_t)batch * t + 1) * c * 2;
}

/* dw[j][g][o][i] = sum over clips and frames of dz[..][64 g + o] * x[.. + j - kernel / 2][64 g + i]; see include/thunder_speech_amd.h */
extern "C" int ts_w2v_posconv_wgrad(const float* dz, const float* x, int32_t batch, int32_t t, int32_t c, int32_t kernel, int32_t groups, float* dw, void* workspace,
                                    void* stream_) {
  if (!dz || !x || !dw || !workspace || batch <= 0 || t <= 0 || c <= 0 || kernel <= 0 || groups <= 0 || c % groups) return TS_EINVAL;
  if (c / groups != 64 || c % 4 || misaligned(workspace) || misaligned(dz) || misaligned(x)) return TS_EUNSUPPORTED;
  TS_STREAM;
  const int prow = t + kernel;
  unsigned short* const xp = static_cast<unsigned short*>(workspace);
  unsigned short* const dz16 = reinterpret_cast<unsigned short*>(static_cast<char*>(workspace) + (((int64_t)batch * prow + 1) * c * 2 + 15) / 16 * 16);
  const long long total_x = ((long long)batch * prow + 1) * c, total_z = ((long long)batch * t + 1) * c;
  hipLaunchKernelGGL(posconv_pad16_kernel, dim3(nblk(total_x / 4)), dim3(256), 0, stream, x, xp, t, c, prow, kernel / 2, total_x);
  hipLaunchKernelGGL(posconv_pad16_kernel, dim3(nblk(total_z / 4)), dim3(256), 0, stream, dz, dz16, t, c, t, 0, total_z);
  PwArgs a{dz16, xp, dw, batch, t, c, kernel, groups};
  hipLaunchKernelGGL(w2v_posconv_wgrad_kernel, dim3((kernel + PW_TAPS - 1) / PW_TAPS, groups), dim3(256), 0, stream, a);
  return hip_status(hipGetLastError());
}

extern "C" int64_t ts_w2v_posconv_train_workspace(int32_t batch, int32_t t, int32_t c, int32_t kernel) {
  if (batch <= 0 || t <= 0 || c <= 0 || kernel <= 0) return TS_EINVAL;
  return ((int64_t)batch * (t + kernel) + 1) * c * 2;
}

/* Positional conv of mixed-precision fine-tuning on the matrix-core kernel; see include/thunder_speech_amd.h */
extern "C" int ts_w2v_posconv_train(const float* src, const float* res, int32_t batch, int32_t t, int32_t c, const void* w_taps_bf16, const float* bias, int32_t kernel,
                                    int32_t groups, int32_t backward, float* y, float* z, void* workspace, void* stream_) {
  if (!src || !res || !w_taps_bf16 || !y || !workspace || batch <= 0 || t <= 0 || c <= 0 || kernel <= 1 || groups <= 0 || c % groups) return TS_EINVAL;
  if (!backward && !bias) return TS_EINVAL;
  const size_t win_lds = (size_t)(PC_TT + kernel - 1) * PC_PITCH;
  if (c / groups != 64 || c % 4 || win_lds > 64 * 1024 || misaligned(workspace) || misaligned(src)) return TS_EUNSUPPORTED;
  TS_STREAM;
  const int prow = t + kernel;
  // forward: kernel / 2 zero rows in front (padding = kernel / 2).  Data gradient: out[s] = sum_j' dz[s + j' - (kernel - 1 - kernel / 2)] Wb[j'] with
  // Wb[j'] = W[kernel - 1 - j']^T -- the same product over a copy padded with kernel - 1 - kernel / 2 rows in front
  const int front = backward ? kernel - 1 - kernel / 2 : kernel / 2;
  unsigned short* const xp = static_cast<unsigned short*>(workspace);
  const long long total = ((long long)batch * prow + 1) * c;
  hipLaunchKernelGGL(posconv_pad16_kernel, dim3(nblk(total / 4)), dim3(256), 0, stream, src, xp, t, c, prow, front, total);
  PcArgs pa{};
  pa.xp = xp; pa.w = static_cast<const unsigned short*>(w_taps_bf16); pa.bias = backward ? nullptr : bias; pa.x = res; pa.y = y;
  pa.t = t; pa.c = c; pa.k = kernel; pa.groups = groups; pa.z = backward ? nullptr : z; pa.plain = backward ? 1 : 0;
  hipLaunchKernelGGL(w2v_posconv_mfma_kernel<false>, dim3((t + PC_TT - 1) / PC_TT, groups, batch), dim3(256), win_lds, stream, pa);
  return hip_status(hipGetLastError());
}
