// WavLM's gated relative-position attention (transformers modeling_wavlm.py WavLMAttention.forward / compute_bias /
// _relative_positions_bucket, reached from huggingface/compatibility.py:31-42 for a WavLM checkpoint).  Declared in
// include/thunder_speech_amd/wavlm.h; everything around the attention core is the wav2vec2 sequence of csrc/w2v_attn.hip.
//
//   ts_wavlm_rel_bias        rb[h][d + t - 1] = E[bucket(d)][h] for d in [-(t - 1), t - 1]: the [H][2t - 1] diagonals of the
//                            position bias, never the [T][T] matrix; the bucket table is built on the host (float32 log there)
//   ts_wavlm_attention_fwd   softmax(q k^T / sqrt(hd) + gate[b][h][i] rb[h][j - i + t - 1] + key mask) v, the gate computed from
//                            the attention's input rows: p = x_h Wg^T + bg, gate = sigmoid(p0..3) (sigmoid(p4..7) const[h] - 1) + 2
//     precision 1, hd 64:   wavlm_flash_attn_kernel, w2v_flash_attn_kernel with the gate in the prologue and the bias window of the
//                            tile staged in LDS next to K / V; the [T][T] scores are never stored
//     precision 0:          scores from the f32 GEMM, one row kernel (gate, bias, mask, softmax), P V on the f32 GEMM
#include "attn_tile.hpp"
#include "w2v_rows.hpp"
#include "thunder_speech_amd/wavlm.h"

namespace ts {

// ---------------------------------------------------------------------------------------------------------------------
// position bias diagonals: one thread per (head, d)
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void wavlm_rel_bias_kernel(const float* __restrict__ embed, const int* __restrict__ abs_bucket, int nb, int md,
                                                             int heads, int t, float* __restrict__ rb) {
  const int n = 2 * t - 1, h = blockIdx.y;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  rb[(size_t)h * n + j] = embed[(size_t)wavlm_bucket(j - (t - 1), nb, md, abs_bucket) * heads + h];
}

// ---------------------------------------------------------------------------------------------------------------------
// precision 0: gate + bias + key mask + softmax over one row of scores [B][H][T][T] per wavefront, in place
// ---------------------------------------------------------------------------------------------------------------------
struct WlRowArgs {
  float* s;                        // [B][H][T][T] raw q . k
  const int* key_len;
  const float* gx;                 // gate input f32 [B][T][ld]
  long long ld;
  const float* wg;                 // [8][hd]
  const float* bg;                 // [8]
  const float* cst;                // [H]
  const float* rb;                 // [H][2T - 1]
  int heads, t, hd;
  float scale;
};

__global__ __launch_bounds__(256) void wavlm_softmax_kernel(const WlRowArgs a) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);     // (head, query) within clip b
  const int lane = threadIdx.x & 63, b = blockIdx.y;
  if (row >= (long long)a.heads * a.t) return;
  const int h = (int)(row / a.t), i = (int)(row - (long long)h * a.t);
  const float* x = a.gx + ((size_t)b * a.t + i) * a.ld + (size_t)h * a.hd;
  float p[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) p[r] = 0.f;
  for (int d = lane; d < a.hd; d += 64) {
    const float xv = x[d];
#pragma unroll
    for (int r = 0; r < 8; ++r) p[r] = fmaf(xv, a.wg[r * a.hd + d], p[r]);
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    for (int o = 32; o > 0; o >>= 1) p[r] += __shfl_xor(p[r], o);      // written out: wave_sum here changes how the eight reductions interleave
    p[r] += a.bg[r];
  }
  const float gate = wavlm_gate(p, a.cst[h]);
  const float* bias = a.rb + (size_t)h * (2 * a.t - 1) + (a.t - 1 - i);     // bias[j] = rb[h][j - i + t - 1]
  float* s = a.s + ((size_t)b * a.heads * a.t + row) * a.t;
  const int n = a.key_len ? key_limit(a.key_len, b, a.t) : a.t;
  const int lim = n > 0 ? n : a.t;                    // no valid key: the softmax runs over all keys (as ts_w2v_attention_fwd)
  float m = -3.0e38f;
  for (int j = lane; j < lim; j += 64) {
    const float v = fmaf(s[j], a.scale, gate * bias[j]);
    s[j] = v;
    m = fmaxf(m, v);
  }
  softmax_row_finish(s, lim, a.t, 1.f, wave_max(m), lane, [s](int j, float v) { s[j] = v; });      // the logits are formed: scale 1
}

// ---------------------------------------------------------------------------------------------------------------------
// Fused gated-bias attention (precision 1, head_dim 64).  To the base sequence of csrc/attn_tile.hpp (w2v_flash_attn_kernel) it adds
//   * the gate of the lane's query in the prologue: lane half h2 dots d = 32 h2 .. 32 h2 + 31 of the query's input row with the
//     8 x 64 weights (staged in LDS once), one exchange with lane ^ 32 completes the 8 projections;
//   * per 64-key tile the window of bias diagonals (stage_window) and the logit formed from it before the maximum (wavlm_logits).
// ---------------------------------------------------------------------------------------------------------------------
struct WaArgs {
  const unsigned short* qkv;       // [B][T][3C] bf16
  unsigned short* ctx;             // [B][T][C] bf16
  const int* key_len;
  const unsigned short* gx;        // gate input bf16 [B][T][ld]
  long long ld;
  const float* wg;                 // [8][64]
  const float* bg;                 // [8]
  const float* cst;                // [H]
  const float* rb;                 // [H][2T - 1]
  int t, c;
  float scale_log2e;
};

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void wavlm_flash_attn_kernel(const WaArgs a) {
  __shared__ __attribute__((aligned(16))) char ks_[AT_KV];
  __shared__ __attribute__((aligned(16))) char vs_[AT_KV];
  __shared__ __attribute__((aligned(16))) float rbs[AT_WIN];
  __shared__ __attribute__((aligned(16))) float wgs[8 * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, head = blockIdx.y;
  const int qw0 = blockIdx.x * AT_QW, q0 = qw0 + wave * 32;
  const size_t rowp = (size_t)3 * a.c;
  const unsigned short* base = a.qkv + (size_t)b * a.t * rowp + (size_t)head * 64;
  const int lim = key_limit<true>(a.key_len, b, a.t);
  const TileLane g = tile_lane(lane);
  const int half = g.half;
  const int query = q0 + g.n32;
  const int qrow = query < a.t ? query : a.t - 1;
  s16x8 qf[4];
  load_row_frags(qf, base + (size_t)qrow * rowp + 8 * half);
  // ---- gate of this lane's query, in log2 units ----
  *reinterpret_cast<f32x2*>(wgs + 2 * tid) = *reinterpret_cast<const f32x2*>(a.wg + 2 * tid);
  __syncthreads();
  float gl;
  {
    const uint4* xp = reinterpret_cast<const uint4*>(a.gx + ((size_t)b * a.t + qrow) * a.ld + (size_t)head * 64 + 32 * half);
    float p[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) p[r] = 0.f;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const uint4 u = xp[v];
      const unsigned w4[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float x0 = bf16_lo(w4[e]), x1 = bf16_hi(w4[e]);
        const int d = 32 * half + 8 * v + 2 * e;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          const f32x2 w = *reinterpret_cast<const f32x2*>(wgs + r * 64 + d);
          p[r] = fmaf(x1, w[1], fmaf(x0, w[0], p[r]));
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) p[r] += __shfl_xor(p[r], 32) + a.bg[r];
    gl = wavlm_gate(p, a.cst[head]) * LOG2E;
  }
  const float* rbh = a.rb + (size_t)head * (2 * a.t - 1);
  f32x16 o[2];
  zero(o[0]); zero(o[1]);
  float m_run = -INFINITY, l_run = 0.f;
  const int wbase = window_base(wave, g);

  for (int k0 = 0; k0 < lim; k0 += AT_KT) {
    __syncthreads();                                                          // the previous tile has been consumed
    stage_kv(ks_, vs_, base, rowp, a.c, a.t, k0, tid);
    stage_window(rbs, rbh, a.t, k0, qw0, tid);
    __syncthreads();
    const bool full = k0 + AT_KT <= lim;                                      // no masked key in this tile (uniform)
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      if (k0 + sub * 32 >= lim) break;                                        // uniform: nothing but masked keys
      f32x16 s = wavlm_logits(qk_subtile(ks_, sub, g, qf), a.scale_log2e, gl, rbs + wbase + 32 * sub);
      if (!full) s = mask_tail(s, k0 + sub * 32 + 8 * half, lim);
      const SoftmaxStep sm = softmax_step<false>(s, m_run, l_run);
      m_run = sm.m; l_run = sm.l;
      rescale(o, sm.alpha);
      acc_tile_t(o, sm.p, vs_, sub, g);
    }
  }
  const float l = l_run + __shfl_xor(l_run, 32);
  const float inv = 1.f / l;
  if (query < a.t) store_bf16(a.ctx + ((size_t)b * a.t + query) * a.c + (size_t)head * 64 + 4 * half, o, inv);
}

}  // namespace ts

using namespace ts;

extern "C" int ts_wavlm_abi_version(void) { return TS_WAVLM_ABI_VERSION; }

extern "C" int ts_wavlm_rel_bias(const float* embed, const int32_t* abs_bucket, int32_t num_buckets, int32_t max_distance, int32_t heads,
                                 int32_t t, float* rel_bias, void* stream_) {
  if (!embed || !abs_bucket || !rel_bias || num_buckets < 2 || max_distance < 0 || heads <= 0 || t <= 0) return TS_EINVAL;
  TS_STREAM;
  hipLaunchKernelGGL(wavlm_rel_bias_kernel, dim3(nblk(2LL * t - 1), heads), dim3(256), 0, stream, embed, abs_bucket,
                     num_buckets, max_distance, heads, t, rel_bias);
  return hip_status(hipGetLastError());
}

extern "C" int64_t ts_wavlm_attention_workspace_bytes(int32_t batch, int32_t t, int32_t heads, int32_t precision) {
  if (batch <= 0 || t <= 0 || heads <= 0) return TS_EINVAL;
  if (precision < 0 || precision > 1) return TS_EUNSUPPORTED;
  return precision ? 0 : (int64_t)batch * heads * t * t * (int64_t)sizeof(float);
}

extern "C" int ts_wavlm_attention_fwd(const void* qkv, int32_t batch, int32_t t, int32_t c, int32_t heads, const int32_t* key_len,
                                      int32_t precision, const void* gate_x, int64_t ld_gate_x, const float* gate_w, const float* gate_b,
                                      const float* gate_const, const float* rel_bias, void* ctx, void* workspace, void* stream_) {
  if (!qkv || !ctx || !gate_x || !gate_w || !gate_b || !gate_const || !rel_bias || batch <= 0 || t <= 0 || c <= 0 || heads <= 0 || c % heads ||
      ld_gate_x < c)
    return TS_EINVAL;
  if (precision < 0 || precision > 1) return TS_EUNSUPPORTED;
  TS_STREAM;
  const int hd = c / heads;
  if (precision) {
    if (hd != 64 || ld_gate_x % 8 || misaligned(gate_x) || misaligned(qkv) || misaligned(gate_w, 7)) return TS_EUNSUPPORTED;
    WaArgs w{};
    w.qkv = static_cast<const unsigned short*>(qkv); w.ctx = static_cast<unsigned short*>(ctx); w.key_len = key_len;
    w.gx = static_cast<const unsigned short*>(gate_x); w.ld = ld_gate_x;
    w.wg = gate_w; w.bg = gate_b; w.cst = gate_const; w.rb = rel_bias;
    w.t = t; w.c = c; w.scale_log2e = LOG2E / sqrtf((float)hd);
    hipLaunchKernelGGL(wavlm_flash_attn_kernel, dim3((t + AT_QW - 1) / AT_QW, heads, batch), dim3(256), 0, stream, w);
    return hip_status(hipGetLastError());
  }
  if (!workspace) return TS_EINVAL;
  float* s = static_cast<float*>(workspace);
  const float* q = static_cast<const float*>(qkv);
  for (int b = 0; b < batch; ++b) {
    const float* qb = q + (size_t)b * t * 3 * c;
    // scores[query][key] = q . k, batched over the heads (head h = columns [h hd, (h+1) hd) of each third of a qkv row)
    if (int st = gemm_f32(stream, false, qb, 3LL * c, 1, hd, 0, qb + c, 1, 3LL * c, hd, 0, s + (size_t)b * heads * t * t, t, (long long)t * t,
                          false, nullptr, t, t, hd, 1, heads, false))
      return st;
  }
  WlRowArgs r{};
  r.s = s; r.key_len = key_len; r.gx = static_cast<const float*>(gate_x); r.ld = ld_gate_x; r.wg = gate_w; r.bg = gate_b; r.cst = gate_const;
  r.rb = rel_bias; r.heads = heads; r.t = t; r.hd = hd; r.scale = 1.f / sqrtf((float)hd);
  hipLaunchKernelGGL(wavlm_softmax_kernel, dim3((unsigned)(((long long)heads * t + 3) / 4), batch), dim3(256), 0, stream, r);
  for (int b = 0; b < batch; ++b) {
    const float* v = q + (size_t)b * t * 3 * c + 2 * c;
    float* out = static_cast<float*>(ctx) + (size_t)b * t * c;
    // ctx[query][d] = sum_key p[query][key] v[key][d], batched over the heads
    if (int st = gemm_f32(stream, false, s + (size_t)b * heads * t * t, t, 1, (long long)t * t, 0, v, 3LL * c, 1, hd, 0, out, c, hd, false, nullptr,
                          t, hd, t, 1, heads, false))
      return st;
  }
  return hip_status(hipGetLastError());
}
