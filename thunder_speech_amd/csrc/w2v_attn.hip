// Self-attention of the wav2vec2 encoder (inference): ts_w2v_attention_fwd = softmax(q k^T * scale [keys >= len masked]) v per (clip, head) over
// the fused qkv rows [B][T][3C], time-major.
//   precision 1, head_dim 64: w2v_flash_attn_kernel<64>, the base sequence of csrc/attn_tile.hpp -- the [T][T] scores are never stored
//                             (attn_flash_launch; ts_mms_attention_fwd, csrc/mms.hip, launches the head_dim 80 instantiation through it)
//   otherwise (precision 0; precision 1 with another head_dim): scores and P V on csrc/gemm_f32.hip, batched over the heads, with
//                             w2v_softmax_kernel (the row softmax of csrc/w2v_rows.hpp) in between; bf16 operands get a bf16 copy of P
#include "attn_tile.hpp"
#include "w2v_rows.hpp"

namespace ts {

// ---------------------------------------------------------------------------------------------------------------------
// attention softmax: one wavefront per (clip, head, query) row of scores [B][H][T][T], in place
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void w2v_softmax_kernel(float* __restrict__ s, const int* __restrict__ key_len, int heads, int t,
                                                          float scale, unsigned short* __restrict__ p16) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.y;
  if (row >= (long long)heads * t) return;
  float* p = s + ((size_t)b * heads * t + row) * t;
  const int n = key_len ? key_limit(key_len, b, t) : t;
  // the reference adds finfo.min to the masked keys: with at least one valid key they get probability exactly 0; with
  // none (len = 0) every key is "equally masked" and the softmax is uniform over all T keys
  const int lim = n > 0 ? n : t;
  unsigned short* q = p16 ? p16 + ((size_t)b * heads * t + row) * t : nullptr;
  softmax_row_finish(p, lim, t, scale, softmax_row_max(p, lim, scale, lane), lane, [p, q](int i, float v) {
    if (q) q[i] = (unsigned short)(pack_bf16(v, 0.f) & 0xffffu);
    else p[i] = v;
  });
}

// ---------------------------------------------------------------------------------------------------------------------
// Fused attention (precision 1, head_dim 64; head_dim 80 for ts_mms_attention_fwd): softmax(q k^T * scale) v without materialising the [T][T] scores.
// This is the base sequence of csrc/attn_tile.hpp (which describes the tile layout and the two geometries) and adds nothing to it: S^T = K Q^T, the
// online softmax with the scale folded into the exponent, O^T += V^T P^T, bf16 output.
// amdgpu_waves_per_eu(4, 4) at either head dimension: the loop is bound by the softmax's quarter-rate exp2, which only other resident waves hide.
// At head_dim 80 the compiler reports 128 VGPRs (48 accumulators, 20 of Q, 16 of scores, the K / V fragments in flight), occupancy 4, 23552 bytes of
// LDS, and 3 spilled VGPRs (16 bytes of scratch); in the generated code the scratch stores sit before the key loop and the reloads after it.  The
// budget of 4 waves forces that spill; (3, 3), which would have none, has not been timed against it.
// ---------------------------------------------------------------------------------------------------------------------
struct FaArgs {
  const unsigned short* qkv;       // [B][T][3C] bf16
  unsigned short* ctx;             // [B][T][C] bf16
  const int* key_len;
  int t, c;
  float scale_log2e;
};

template <int HD>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void w2v_flash_attn_kernel(const FaArgs a) {
  using G = AttnGeom<HD>;
  __shared__ __attribute__((aligned(16))) char ks_[AT_KT * G::RP];
  __shared__ __attribute__((aligned(16))) char vs_[AT_KT * G::TP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, head = blockIdx.y;
  const int q0 = blockIdx.x * AT_QW + wave * 32;
  const size_t rowp = (size_t)3 * a.c;
  const unsigned short* base = a.qkv + (size_t)b * a.t * rowp + (size_t)head * HD;
  const int lim = key_limit<true>(a.key_len, b, a.t);
  const TileLane g = tile_lane<G::TP>(lane);
  const int query = q0 + g.n32;
  zero_pad<HD, G::TP>(vs_, AT_KT, tid, 256);                                  // the loop's first barrier orders it before any read
  s16x8 qf[HD / 16];
  load_row_frags(qf, base + (size_t)(query < a.t ? query : a.t - 1) * rowp + 8 * g.half);
  f32x16 o[(HD + 31) / 32];
#pragma unroll
  for (int mt = 0; mt < (HD + 31) / 32; ++mt) zero(o[mt]);
  float m_run = -INFINITY, l_run = 0.f;

  // (A register-prefetched, double-buffered variant of this loop was measured SLOWER: 176 VGPRs halve the occupancy, and this
  // kernel is bound by the softmax VALU work -- exp2 runs at quarter rate -- which only other resident waves can hide.)
  for (int k0 = 0; k0 < lim; k0 += AT_KT) {
    __syncthreads();                                                          // the previous tile has been consumed
    stage_kv<HD, G::RP, G::TP>(ks_, vs_, base, rowp, a.c, a.t, k0, tid);
    __syncthreads();
    const bool full = k0 + AT_KT <= lim;                                      // no masked key in this tile (uniform)
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      if (k0 + sub * 32 >= lim) break;                                        // uniform: nothing but masked keys
      f32x16 s = qk_subtile<G::RP>(ks_, sub, g, qf);
      if (!full) s = mask_tail(s, k0 + sub * 32 + 8 * g.half, lim);
      const SoftmaxStep sm = softmax_step<true>(s, m_run, l_run, a.scale_log2e);
      m_run = sm.m; l_run = sm.l;
      rescale(o, sm.alpha);
      acc_tile_t<G::TP>(o, sm.p, vs_, sub, g);
    }
  }
  const float l = l_run + __shfl_xor(l_run, 32);
  const float inv = 1.f / l;
  if (query < a.t) store_bf16<HD>(a.ctx + ((size_t)b * a.t + query) * a.c + (size_t)head * HD + 4 * g.half, o, inv);
}

template <int HD>
static int flash_launch(const void* qkv, int32_t batch, int32_t t, int32_t c, int32_t heads, const int32_t* key_len, void* ctx, hipStream_t stream) {
  FaArgs f{};
  f.qkv = static_cast<const unsigned short*>(qkv); f.ctx = static_cast<unsigned short*>(ctx); f.key_len = key_len;
  f.t = t; f.c = c; f.scale_log2e = LOG2E / sqrtf((float)HD);
  hipLaunchKernelGGL(w2v_flash_attn_kernel<HD>, dim3((t + AT_QW - 1) / AT_QW, heads, batch), dim3(256), 0, stream, f);
  return hip_status(hipGetLastError());
}

int attn_flash_launch(int hd, const void* qkv, int32_t batch, int32_t t, int32_t c, int32_t heads, const int32_t* key_len, void* ctx, hipStream_t stream) {
  return hd == 64 ? flash_launch<64>(qkv, batch, t, c, heads, key_len, ctx, stream) : flash_launch<80>(qkv, batch, t, c, heads, key_len, ctx, stream);
}

}  // namespace ts

using namespace ts;

extern "C" int64_t ts_w2v_attention_workspace_bytes(int32_t batch, int32_t t, int32_t heads, int32_t precision) {
  if (batch <= 0 || t <= 0 || heads <= 0) return TS_EINVAL;
  return (int64_t)batch * heads * t * t * (sizeof(float) + (precision ? 2 : 0));
}

extern "C" int ts_w2v_attention_fwd(const void* qkv, int32_t batch, int32_t t, int32_t c, int32_t heads, const int32_t* key_len,
                                    int32_t precision, void* ctx, void* workspace, void* stream_) {
  if (!qkv || !ctx || !workspace || batch <= 0 || t <= 0 || c <= 0 || heads <= 0 || c % heads) return TS_EINVAL;
  if (precision < 0 || precision > 1) return TS_EUNSUPPORTED;
  TS_STREAM;
  const int hd = c / heads;
  const bool bf = precision != 0;
  if (bf && hd == 64 && c % 8 == 0) return attn_flash_launch(64, qkv, batch, t, c, heads, key_len, ctx, stream);
  const size_t es = bf ? 2 : 4;
  float* s = static_cast<float*>(workspace);
  unsigned short* p16 = bf ? reinterpret_cast<unsigned short*>(s + (size_t)batch * heads * t * t) : nullptr;
  for (int b = 0; b < batch; ++b) {
    const char* q = static_cast<const char*>(qkv) + (size_t)b * t * 3 * c * es;
    // scores[query][key] = q . k : batched over the heads (head h = columns [h hd, (h+1) hd) of each third of a qkv row)
    if (int st = gemm_nt(stream, bf, t, t, hd, q, 3LL * c, hd, q + (size_t)c * es, 3LL * c, hd, s + (size_t)b * heads * t * t, t,
                         (long long)t * t, 0.f, heads))
      return st;
  }
  hipLaunchKernelGGL(w2v_softmax_kernel, dim3((unsigned)(((long long)heads * t + 3) / 4), batch), dim3(256), 0, stream, s, key_len, heads, t,
                     1.f / sqrtf((float)hd), p16);
  for (int b = 0; b < batch; ++b) {
    const char* v = static_cast<const char*>(qkv) + ((size_t)b * t * 3 * c + 2 * c) * es;
    const void* p = bf ? static_cast<const void*>(p16 + (size_t)b * heads * t * t) : static_cast<const void*>(s + (size_t)b * heads * t * t);
    void* out = static_cast<char*>(ctx) + (size_t)b * t * c * es;
    // ctx[query][d] = sum_key p[query][key] v[key][d], batched over the heads (head h = columns [h hd, (h+1) hd) of a v / ctx row); bf16 in -> bf16 out
    if (int st = gemm_f32(stream, bf, p, t, 1, (long long)t * t, 0, v, 3LL * c, 1, hd, 0, out, c, hd, bf, nullptr, t, hd, t, 1, heads, false)) return st;
  }
  return hip_status(hipGetLastError());
}
