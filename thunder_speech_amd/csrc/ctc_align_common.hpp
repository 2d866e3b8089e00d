// What the two Viterbi aligners (csrc/ctc_align.hip, csrc/ctc_align_long.hip) share, so that "the same arithmetic" is the same text: the
// LDS-ordering barrier, a path frame's log-probability in f64 and the epilogue (path, spans, score, span sums).
#pragma once
#include "ts_common.hpp"

namespace ts {

constexpr float ALIGN_NEG_INF = -__builtin_huge_valf();

// workgroup barrier that orders LDS traffic only (csrc/ctc.hip: __syncthreads() would also wait for the emission prefetch ring at every step)
__device__ __forceinline__ void align_lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// log_softmax(lg[:, t])[tok]: maximum in f32 (exact), the sum of exponentials, the logarithm and the difference in f64, rounded to f32 once.
// Batches of 8 independent loads, as the log-sum-exp prologue of csrc/ctc.hip.
__device__ __forceinline__ float frame_logp(const float* lg, int V, int pitch, int t, int tok) {
  float m = lg[t];
  for (int v0 = 1; v0 < V; v0 += 8) {
    float x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = lg[(size_t)min(v0 + u, V - 1) * pitch + t];
#pragma unroll
    for (int u = 0; u < 8; ++u) m = fmaxf(m, x[u]);
  }
  double sum = 0.0;
  for (int v0 = 0; v0 < V; v0 += 8) {
    float x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = lg[(size_t)min(v0 + u, V - 1) * pitch + t];
#pragma unroll
    for (int u = 0; u < 8; ++u) sum += (v0 + u < V) ? exp((double)x[u] - (double)m) : 0.0;
  }
  return (float)((double)lg[(size_t)tok * pitch + t] - (double)m - log(sum));
}

// The epilogue of an aligner's workgroup, behind the backtrace and a __syncthreads(): the path's cells in parallel over the frames (token,
// log-probability, span boundaries), the score by a wave / workgroup reduction, then one thread per label sums its span in frame order.
// st [n_frames]: the path's state per frame; lpw [n_frames]: scratch for the path's log-probabilities; red: 16 floats of LDS; token(s): the class of
// state s.  Every thread of the workgroup calls it.
template <class Token>
__device__ __forceinline__ void align_epilogue(const float* lg, int V, int pitch, int n_frames, int s_max, int T, int S, int L, bool feasible, const int* st,
                                               float* lpw, int* path, int* spans, float* span_logp, float* score, float* red, Token token) {
  const int lane = threadIdx.x, wave = threadIdx.x >> 6, NT = blockDim.x;
  const int Tp = feasible ? T : 0;
  float part = 0.f;
  for (int t = lane; t < Tp; t += NT) {
    const int s = min(max(st[t], 0), L - 1);
    const int sp = t > 0 ? st[t - 1] : -1, sn = t + 1 < Tp ? st[t + 1] : -1;
    const int tok = token(s);
    const float lp = frame_logp(lg, V, pitch, t, tok);
    path[t] = tok;
    lpw[t] = lp;
    part += lp;
    if (s & 1) {
      if (sp != s) spans[(s >> 1) * 2] = t;
      if (sn != s) spans[(s >> 1) * 2 + 1] = t + 1;
    }
  }
  for (int t = Tp + lane; t < n_frames; t += NT) path[t] = -1;
  part = wave_sum(part);
  if ((lane & 63) == 0) red[wave] = part;
  __syncthreads();                                 // and the spans and log-probabilities above are visible to the workgroup
  if (lane == 0) {
    float sc = 0.f;
    for (int w = 0; w < (NT >> 6); ++w) sc += red[w];
    *score = feasible ? sc : ALIGN_NEG_INF;
  }
  // one thread per label: the span's log-probabilities summed in frame order, 8 independent loads at a time
  const int Sp = feasible ? S : 0;
  for (int j = lane; j < s_max; j += NT) {
    if (j >= Sp) {
      spans[j * 2] = 0; spans[j * 2 + 1] = 0; span_logp[j] = 0.f;
      continue;
    }
    const int t0 = min(max(spans[j * 2], 0), Tp), t1 = min(max(spans[j * 2 + 1], t0), Tp);
    float sum = 0.f;
    for (int t = t0; t < t1; t += 8) {
      float x[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) x[u] = lpw[min(t + u, t1 - 1)];
#pragma unroll
      for (int u = 0; u < 8; ++u) sum += (t + u < t1) ? x[u] : 0.f;
    }
    span_logp[j] = sum;
  }
}

}  // namespace ts
