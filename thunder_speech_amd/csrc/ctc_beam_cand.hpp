// What the two CTC beam searches share (csrc/ctc_beam.hip, csrc/ctc_beam_lm.hip): the limits, the prefix hash, the LDS-only barrier and the
// frame-candidate pre-pass.  Included AFTER the including source's `#pragma clang fp contract(off) reassociate(off)`: the f64 sums and the
// quotient of beam_prob are the specification's in both.  The kernel sits in an unnamed namespace: each including source gets its own copy.
#pragma once
#include "ts_common.hpp"

namespace ts {
namespace {

constexpr int BEAM_MAX = 64;                          // beam_width, token_cap and n_best at most
constexpr float BEAM_NEG_INF = -__builtin_huge_valf();
constexpr int BEAM_NONE = 0x7fffffff;
constexpr int BEAM_FIN = 64;                          // final nodes per utterance in the workspace
constexpr int BEAM_ROW = 64;                          // up to this many classes the pre-pass leaves every class's probability per frame

__host__ __device__ constexpr int beam_even(int x) { return (x + 1) & ~1; }

// workgroup barrier that orders LDS traffic only (csrc/ctc_align.hip: __syncthreads() would also wait for the record prefetch ring at every step)
__device__ __forceinline__ void beam_lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

__device__ __forceinline__ unsigned long long beam_mix(unsigned long long h, int c) {
  unsigned long long z = h + 0x9E3779B97F4A7C15ull * (unsigned long long)(unsigned)(c + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the probability of a logit x of a frame with maximum m and sum of exponentials `sum`: the one expression both kernels use
__device__ __forceinline__ double beam_prob(float x, float m, double sum) { return exp((double)x - (double)m) / sum; }

// Frame records, [B][n_frames][cap + 2]: record 0 the blank, records 1 .. cap the kept classes by (logit descending, class ascending), record
// cap + 1 the normaliser (id = bits of the f32 maximum, p = the f64 sum).  A record without a class (fewer comparable logits than cap) is (-2, 0).
// With V <= BEAM_ROW also prow [B][n_frames][BEAM_ROW]: the probability of every class, for the stay candidates' p[last].
__global__ __launch_bounds__(256) void ctc_beam_cand_kernel(const float* __restrict__ logits, int V, int n_frames, int pitch,
                                                            const int* __restrict__ input_len, int blank, int cap, double* __restrict__ cp,
                                                            int* __restrict__ cid, double* __restrict__ prow) {
  const int b = blockIdx.y, lane = threadIdx.x & 63, t = blockIdx.x * 4 + (threadIdx.x >> 6);
  int T = input_len ? input_len[b] : n_frames;
  T = T < 0 ? 0 : (T > n_frames ? n_frames : T);
  if (t >= T) return;                                  // wave-uniform
  const float* lg = logits + (size_t)b * V * pitch + t;
  const size_t at = ((size_t)b * n_frames + t) * (cap + 2);
  double* const p_o = cp + at;
  int* const id_o = cid + at;
  float m = BEAM_NEG_INF;
  for (int c = lane; c < V; c += 64) m = fmaxf(m, lg[(size_t)c * pitch]);
  m = wave_max(m);
  double sum = 0.0;
  for (int c = lane; c < V; c += 64) sum += exp((double)lg[(size_t)c * pitch] - (double)m);
  sum = wave_sum(sum);
  if (V <= BEAM_ROW && lane < V) prow[((size_t)b * n_frames + t) * BEAM_ROW + lane] = beam_prob(lg[(size_t)lane * pitch], m, sum);
  if (lane == 0) {
    p_o[0] = beam_prob(lg[(size_t)blank * pitch], m, sum);
    id_o[0] = blank;
    p_o[cap + 1] = sum;
    id_o[cap + 1] = __float_as_int(m);
  }
  float px = __builtin_huge_valf();                    // the previous winner: everything comes after (+inf, -1)
  int pc = -1;
  for (int k = 0; k < cap; ++k) {
    float bx = BEAM_NEG_INF;
    int bc = BEAM_NONE;
    for (int c = lane; c < V; c += 64) {
      const float x = lg[(size_t)c * pitch];
      const bool after = x < px || (x == px && c > pc);
      const bool better = x > bx || (x == bx && c < bc);
      if (c != blank && after && better) { bx = x; bc = c; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ox = __shfl_xor(bx, o);
      const int oc = __shfl_xor(bc, o);
      if (oc != BEAM_NONE && (bc == BEAM_NONE || ox > bx || (ox == bx && oc < bc))) { bx = ox; bc = oc; }
    }
    const bool found = bc != BEAM_NONE;
    if (lane == 0) {
      id_o[1 + k] = found ? bc : -2;
      p_o[1 + k] = found ? beam_prob(bx, m, sum) : 0.0;
    }
    px = found ? bx : BEAM_NEG_INF;                    // nothing comes after (-inf, BEAM_NONE)
    pc = bc;
  }
}

}  // namespace
}  // namespace ts
