// Recordings longer than one forward pass, for gfx950: the two plumbing launches around the forward.  No reference counterpart (the reference's
// predict takes one batch that fits one pass, module.py:88-100).  ABI: include_open/thunder_speech_amd/longform.h; the window plan that fills the
// tables is host arithmetic (thunder_speech_amd/longform.py).
//
// ts_longform_gather exists because predict()'s zero-copy inference graph is keyed by the input's address: every batch of windows enters the model
// through ONE staging buffer, and this launch fills it (rows past the last window and samples past a recording's end as zeros, so that every
// window is full length and one [batch, chunk] signature serves all batches).
// ts_longform_stitch turns the windows' logits back into one logit sequence per recording: window w owns the global frames [cut_lo, cut_hi) and
// one workgroup per (window, class) copies that range, so every output cell has exactly one writer: no search, no atomics, both sides read and
// written along time.
#include "ts_common.hpp"

#include "thunder_speech_amd/longform.h"

namespace ts {

constexpr int LF_TH = 256;

// one thread per 4 samples of a row
template <bool VEC>
__global__ __launch_bounds__(LF_TH) void longform_gather_kernel(const float* __restrict__ audio, const long long* __restrict__ rec_begin, int n_recordings,
                                                                const long long* __restrict__ windows, int n_windows, float* __restrict__ out, int chunk) {
  const int row = blockIdx.y;
  const long long i0 = ((long long)blockIdx.x * LF_TH + threadIdx.x) * 4;
  if (i0 >= chunk) return;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (row < n_windows) {
    const long long rec = windows[2 * row], start = windows[2 * row + 1];
    if (rec >= 0 && rec < n_recordings) {
      const long long begin = rec_begin[rec], n = rec_begin[rec + 1] - begin;
      const long long p0 = start + i0;                                     // position within the recording of this thread's first sample
      const float* const src = audio + begin + p0;
      if (p0 >= 0 && p0 + 4 <= n && i0 + 4 <= chunk && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(src);
        v[0] = x[0]; v[1] = x[1]; v[2] = x[2]; v[3] = x[3];
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (p0 + u >= 0 && p0 + u < n && i0 + u < chunk) v[u] = src[u];
      }
    }
  }
  float* const dst = out + (size_t)row * chunk + i0;
  if (VEC) {                                                               // chunk % 4 == 0 and out 16-byte aligned: every row segment is whole
    *reinterpret_cast<f32x4*>(dst) = f32x4{v[0], v[1], v[2], v[3]};
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (i0 + u < chunk) dst[u] = v[u];
  }
}

__device__ __forceinline__ float lf_load(const float* p, size_t i) { return p[i]; }
__device__ __forceinline__ float lf_load(const unsigned short* p, size_t i) { return bf16_to_f32(p[i]); }

// workgroup (w, v): out[rec][v][lo .. hi) = win[w][v][lo - g_w ..), and zeros behind the recording's last window
template <class In>
__global__ __launch_bounds__(LF_TH) void longform_stitch_kernel(const In* __restrict__ win, int n_windows, int n_classes, int frames, const int* __restrict__ cuts,
                                                                float* __restrict__ out, int n_recordings, int pitch, int* __restrict__ lengths) {
  const int w = blockIdx.x, v = blockIdx.y;
  const int rec = cuts[4 * w], g = cuts[4 * w + 1];
  if (rec < 0 || rec >= n_recordings) return;
  const int first = max(g, 0), end = (int)min((long long)g + frames, (long long)pitch);
  const int lo = min(max(cuts[4 * w + 2], first), max(end, first)), hi = min(max(cuts[4 * w + 3], lo), max(end, lo));
  const bool last = w + 1 == n_windows || cuts[4 * (w + 1)] != rec;
  const In* const src = win + ((size_t)w * n_classes + v) * frames;
  float* const dst = out + ((size_t)rec * n_classes + v) * pitch;
  for (int t = lo + threadIdx.x; t < hi; t += LF_TH) dst[t] = lf_load(src, (size_t)(t - g));
  if (last) {
    for (int t = hi + threadIdx.x; t < pitch; t += LF_TH) dst[t] = 0.f;
    if (v == 0 && threadIdx.x == 0) lengths[rec] = hi;
  }
}

}  // namespace ts

extern "C" int ts_longform_abi_version(void) { return TS_LONGFORM_ABI_VERSION; }

extern "C" int ts_longform_gather(const float* audio, const int64_t* rec_begin, int32_t n_recordings, const int64_t* windows, int32_t n_windows,
                                  float* out, int32_t batch, int32_t chunk, void* stream_) {
  using namespace ts;
  if (!audio || !rec_begin || !windows || !out) return TS_EINVAL;
  if (n_recordings <= 0 || n_windows < 0 || batch <= 0 || n_windows > batch || chunk <= 0) return TS_EINVAL;
  if (misaligned(audio, 3) || misaligned(out, 3) || misaligned(rec_begin, 7) || misaligned(windows, 7)) return TS_EUNSUPPORTED;
  if (batch > 65535) return TS_EUNSUPPORTED;
  TS_STREAM;
  const dim3 grid(nblk(((long long)chunk + 3) / 4), (unsigned)batch);
  const long long* const rb = reinterpret_cast<const long long*>(rec_begin);
  const long long* const wn = reinterpret_cast<const long long*>(windows);
  if (chunk % 4 == 0 && !misaligned(out))
    hipLaunchKernelGGL(longform_gather_kernel<true>, grid, dim3(LF_TH), 0, stream, audio, rb, n_recordings, wn, n_windows, out, chunk);
  else
    hipLaunchKernelGGL(longform_gather_kernel<false>, grid, dim3(LF_TH), 0, stream, audio, rb, n_recordings, wn, n_windows, out, chunk);
  return hip_status(hipGetLastError());
}

extern "C" int ts_longform_stitch(const void* win, int32_t in_bf16, int32_t n_windows, int32_t n_classes, int32_t frames_per_window,
                                  const int32_t* cuts, float* out, int32_t n_recordings, int32_t pitch, int32_t* lengths, void* stream_) {
  using namespace ts;
  if (!win || !cuts || !out || !lengths) return TS_EINVAL;
  if (n_windows <= 0 || n_classes <= 0 || frames_per_window <= 0 || n_recordings <= 0 || pitch <= 0 || n_classes > 65535) return TS_EINVAL;
  if (misaligned(win, in_bf16 ? 1 : 3) || misaligned(cuts, 3) || misaligned(out, 3) || misaligned(lengths, 3)) return TS_EUNSUPPORTED;
  TS_STREAM;
  const dim3 grid((unsigned)n_windows, (unsigned)n_classes);
  if (in_bf16)
    hipLaunchKernelGGL(longform_stitch_kernel<unsigned short>, grid, dim3(LF_TH), 0, stream, static_cast<const unsigned short*>(win), n_windows,
                       n_classes, frames_per_window, cuts, out, n_recordings, pitch, lengths);
  else
    hipLaunchKernelGGL(longform_stitch_kernel<float>, grid, dim3(LF_TH), 0, stream, static_cast<const float*>(win), n_windows, n_classes,
                       frames_per_window, cuts, out, n_recordings, pitch, lengths);
  return hip_status(hipGetLastError());
}
