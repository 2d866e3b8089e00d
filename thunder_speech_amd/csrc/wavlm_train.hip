// Mixed-precision WavLM FINE-TUNING: the gated relative-position attention of transformers' WavLMAttention (modeling_wavlm.py forward /
// compute_bias, reached through huggingface/compatibility.py:31-42 under the reference's training_step, module.py:102-127) forward and backward
// without the [T][T] matrices, plus the gate and the position-bias embedding with their gradients.  Declared in
// include/thunder_speech_amd_wavlm_train.h.  Derived from csrc/w2v_attn_train.hip (which stays the wav2vec2 path) and csrc/wavlm.hip:
//
//   ts_wavlm_gate_fwd       g[b][h][i] = ga (gb c_h - 1) + 2, ga = sigmoid(p0..3), gb = sigmoid(p4..7), p = x_h W^T + beta   (ga, gb kept)
//   ts_wavlm_gate_bwd       dp0..3 = dg (gb c - 1) ga (1 - ga), dp4..7 = dg ga c gb (1 - gb): dx_h = dp W (written), dW / dbeta / dc from per-wave
//                           partials summed in a fixed order (wavlm_gate_sum_kernel)
//   ts_wavlm_attention_train_fwd   attn_fwd_train_kernel + the bias of wavlm_flash_attn_kernel: the logit s q.k + g[i] rb[j - i + t - 1] (log2
//                           units) formed before the running maximum, the tile's diagonals staged in LDS; ctx f32 and lse2 (bias included)
//   ts_wavlm_attention_train_bwd   rowdot, dQ and dKV kernels of the wav2vec2 path rebuilding P with the bias, and
//                           dg[b][h][i] = sum_j dS_ij rb[j - i + t - 1]          (dQ kernel: the lane owns query i)
//                           drb[h][d + t - 1] = sum_b sum_i g_i dS[i][i + d]      (dKV kernel: the wave's bf16 dS tile [32 q][64 k] read back along
//                           its 95 diagonals, one record per (clip, head, key tile, 32-query tile); wavlm_drb_sum_kernel adds the records of a
//                           diagonal in a fixed order)
//   ts_wavlm_rel_bias_bwd   dE[k][h] = sum over the diagonals d with bucket(d) = k of drb[h][d + t - 1]: one wave per (bucket, head), a gather
// No float atomics anywhere: two calls give the same bits.
#include "ts_common.hpp"
#include "ts_philox.hpp"
#include "thunder_speech_amd_wavlm_train.h"

namespace ts {

namespace {

constexpr int WT_KT = 64;          // keys per staged tile
constexpr int WT_PITCH = 144;      // bytes per staged bf16 row: 64 bf16 + 16
constexpr int WT_QW = 128;         // queries per workgroup of the forward / dQ kernels (4 waves x 32)
constexpr int WT_WIN = WT_QW + WT_KT;   // 191 diagonals of a 128 x 64 tile, rounded up
constexpr int WT_DG = 95;          // diagonals of a 32 x 64 tile: the dKV kernel's per-wave window and drb record
constexpr float LOG2E = 1.4426950408889634f;

__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + __expf(-x)); }

struct WtArgs {
  const unsigned short* qkv;       // [B][T][3C] bf16
  const int* key_len;
  const float* gate;               // [B][H][T]
  const float* rb;                 // [H][2T - 1]
  float* ctx;                      // forward: [B][T][C] f32
  float* lse2;                     // [B][H][T]
  const unsigned short* dout;      // backward: [B][T][C] bf16
  const float* dsum;               // backward: D [B][H][T]
  float* dqkv;                     // backward: [B][T][3C] f32
  float* dgate;                    // backward: [B][H][T]
  float* dparts;                   // backward: drb records [B][H][nkt][nqt][95]
  int t, c, heads, nkt, nqt;
  float scale_log2e, scale;        // log2(e) / sqrt(hd), 1 / sqrt(hd)
  float p_drop, keep_scale;        // dropout probability, 1 / (1 - p)
  const unsigned* mask;            // keep bits of the [B H T][T] dropout stream (wt_mask_kernel); NULL when p_drop == 0
};

__device__ __forceinline__ int wt_lim(const WtArgs& a, int b) {
  if (!a.key_len) return a.t;
  const int n = a.key_len[b] < a.t ? a.key_len[b] : a.t;
  return n > 0 ? n : 0;            // no valid key: every probability 0 (the training convention of ts_w2v_attention_train_fwd)
}

// the dropout mask as a bitstring, drawn once per call: bit e set iff element e of the logical [B H T][T] matrix is kept -- ts_train_dropout's rule
// (u01(word e & 3 of Philox block e >> 2) >= p), the same stream as ts_w2v_attention_train_fwd
__global__ __launch_bounds__(256) void wt_mask_kernel(unsigned* __restrict__ mask, long long n_words, unsigned long long seed, float p) {
  const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
  if (w >= n_words) return;
  unsigned bits = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const Philox4 r = philox(seed, PHILOX_DROPOUT, (unsigned long long)w * 8 + j);
#pragma unroll
    for (int q = 0; q < 4; ++q) bits |= (u01(r.v[q]) >= p ? 1u : 0u) << (4 * j + q);
  }
  mask[w] = bits;
}

__device__ __forceinline__ unsigned keep8(const unsigned* __restrict__ mask, unsigned long long e0) {
  const unsigned long long w = e0 >> 5;
  const unsigned long long both = ((unsigned long long)mask[w + 1] << 32) | mask[w];
  return (unsigned)(both >> (e0 & 31)) & 0xffu;
}

// K and V rows k0 .. k0 + 63 of one (clip, head) into LDS (rows past t clamped to t - 1: never stored, their probabilities are 0)
__device__ __forceinline__ void stage_kv(char* ks_, char* vs_, const unsigned short* base, size_t rowp, int c, int t, int k0, int tid) {
#pragma unroll
  for (int rep = 0; rep < 2; ++rep) {
    const int chunk = tid + 256 * rep, r = chunk >> 3, cc = chunk & 7;
    const int key = k0 + r < t ? k0 + r : t - 1;
    const unsigned short* src = base + (size_t)key * rowp + cc * 8;
    *reinterpret_cast<uint4*>(ks_ + r * WT_PITCH + cc * 16) = *reinterpret_cast<const uint4*>(src + c);
    *reinterpret_cast<uint4*>(vs_ + r * WT_PITCH + cc * 16) = *reinterpret_cast<const uint4*>(src + 2 * c);
  }
}

// rb[h][d + t - 1] for d = dlo + s, s < n, into LDS (slots outside [-(t - 1), t - 1] clamped: they belong to clamped keys / queries)
__device__ __forceinline__ float rb_at(const float* rbh, int t, int d) {
  int j = d + t - 1;
  j = j < 0 ? 0 : (j > 2 * t - 2 ? 2 * t - 2 : j);
  return rbh[j];
}

// ---------------------------------------------------------------------------------------------------------------------
// forward: attn_fwd_train_kernel with the gated bias in the logit
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void wt_fwd_kernel(const WtArgs a) {
  __shared__ __attribute__((aligned(16))) char ks_[WT_KT * WT_PITCH];
  __shared__ __attribute__((aligned(16))) char vs_[WT_KT * WT_PITCH];
  __shared__ __attribute__((aligned(16))) float rbs[WT_WIN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, head = blockIdx.y;
  const int qw0 = blockIdx.x * WT_QW, q0 = qw0 + wave * 32;
  const size_t rowp = (size_t)3 * a.c;
  const unsigned short* base = a.qkv + (size_t)b * a.t * rowp + (size_t)head * 64;
  const int lim = wt_lim(a, b);
  const int half = lane >> 5, n32 = lane & 31;
  const int query = q0 + n32;
  const int qrow = query < a.t ? query : a.t - 1;
  const bool drop = a.p_drop > 0.f;
  const size_t bh = (size_t)b * a.heads + head;
  const unsigned long long erow = ((unsigned long long)bh * a.t + qrow) * (unsigned long long)a.t;
  s16x8 qf[4];
  {
    const uint4* qp = reinterpret_cast<const uint4*>(base + (size_t)qrow * rowp + 8 * half);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = __builtin_bit_cast(s16x8, qp[2 * ks]);
  }
  const float gl = a.gate[bh * a.t + qrow] * LOG2E;
  const float* rbh = a.rb + (size_t)head * (2 * a.t - 1);
  f32x16 o[2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int i = 0; i < 16; ++i) o[mt][i] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;
  const int pm = (n32 & ~12) | ((n32 & 4) << 1) | ((n32 & 8) >> 1);          // K row order: bits 2 and 3 swapped
  const int q4 = (lane >> 2) & 3, gq = (lane >> 4) & 1, p4 = lane & 3;
  const int v_off = (8 * half + q4) * WT_PITCH + (16 * gq + 4 * p4) * 2;     // transposing read of the V tile
  // window slot of (key k0 + kk, query qw0 + qq) is kk - qq + WT_QW - 1
  const int wbase = WT_QW - 1 - (wave * 32 + n32) + 8 * half;

  for (int k0 = 0; k0 < lim; k0 += WT_KT) {
    __syncthreads();
    stage_kv(ks_, vs_, base, rowp, a.c, a.t, k0, tid);
    if (tid < WT_WIN) rbs[tid] = rb_at(rbh, a.t, k0 - qw0 - (WT_QW - 1) + tid);
    __syncthreads();
    const bool full = k0 + WT_KT <= lim;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      if (k0 + sub * 32 >= lim) break;
      f32x16 s;
#pragma unroll
      for (int i = 0; i < 16; ++i) s[i] = 0.f;
      const char* kr = ks_ + (sub * 32 + pm) * WT_PITCH + half * 16;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const s16x8*>(kr + ks * 32), qf[ks], s, 0, 0, 0);
      // accumulator register i <-> key kbase + 16 (i / 8) + i % 8
      const int kbase = k0 + sub * 32 + 8 * half;
      const float* wr = rbs + wbase + 32 * sub;
#pragma unroll
      for (int i = 0; i < 16; ++i) s[i] = fmaf(s[i], a.scale_log2e, gl * wr[16 * (i >> 3) + (i & 7)]);
      if (!full) {
#pragma unroll
        for (int i = 0; i < 16; ++i)
          if (kbase + 16 * (i >> 3) + (i & 7) >= lim) s[i] = -INFINITY;
      }
      float mx = s[0];
#pragma unroll
      for (int i = 1; i < 16; ++i) mx = fmaxf(mx, s[i]);
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float m_new = fmaxf(m_run, mx);                                   // finite: the first sub-tile holds key 0
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      float rs = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) { s[i] = __builtin_amdgcn_exp2f(s[i] - m_new); rs += s[i]; }
      l_run = l_run * alpha + rs;                                             // the normaliser counts every key, dropped or not
      m_run = m_new;
      if (drop) {
        const unsigned k_lo = keep8(a.mask, erow + kbase), k_hi = keep8(a.mask, erow + kbase + 16);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          s[i] = (k_lo >> i) & 1u ? s[i] * a.keep_scale : 0.f;
          s[8 + i] = (k_hi >> i) & 1u ? s[8 + i] * a.keep_scale : 0.f;
        }
      }
      if (__any(alpha != 1.f)) {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
          for (int i = 0; i < 16; ++i) o[mt][i] *= alpha;
      }
#pragma unroll
      for (int ks2 = 0; ks2 < 2; ++ks2) {
        const unsigned p01 = pack_bf16(s[8 * ks2 + 0], s[8 * ks2 + 1]), p23 = pack_bf16(s[8 * ks2 + 2], s[8 * ks2 + 3]);
        const unsigned p45 = pack_bf16(s[8 * ks2 + 4], s[8 * ks2 + 5]), p67 = pack_bf16(s[8 * ks2 + 6], s[8 * ks2 + 7]);
        const s16x8 pb = __builtin_bit_cast(s16x8, uint4{p01, p23, p45, p67});
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
          const char* va = vs_ + (sub * 32 + 16 * ks2) * WT_PITCH + v_off + 64 * mt;
          const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((TS_LDS s16x4*)((TS_LDS char*)va));
          const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((TS_LDS s16x4*)((TS_LDS char*)va + 4 * WT_PITCH));
          const s16x8 vf = s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          o[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pb, o[mt], 0, 0, 0);
        }
      }
    }
  }
  const float l = l_run + __shfl_xor(l_run, 32);
  const float inv = l > 0.f ? 1.f / l : 0.f;
  if (query < a.t) {
    float* dst = a.ctx + ((size_t)b * a.t + query) * a.c + (size_t)head * 64 + 4 * half;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int g = 0; g < 4; ++g)       // accumulator registers 4g .. 4g+3 <-> d = 32 mt + 8 g + 4 half + 0..3
        *reinterpret_cast<f32x4*>(dst + 32 * mt + 8 * g) = f32x4{o[mt][4 * g] * inv, o[mt][4 * g + 1] * inv, o[mt][4 * g + 2] * inv, o[mt][4 * g + 3] * inv};
    if (half == 0) a.lse2[bh * a.t + query] = l > 0.f ? m_run + __builtin_amdgcn_logf(l) : INFINITY;      // v_log_f32 = log2
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// backward, part 0: bf16 copy of dO and D[b][h][q] = sum_d dO[q][d] O[q][d] (one wave per (b, q) row)
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void wt_rowdot_kernel(const float* __restrict__ dout, const float* __restrict__ ctx, unsigned short* __restrict__ dout16,
                                                        float* __restrict__ dsum, long long rows, int t, int c, int heads) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const long long b = row / t;
  const int q = (int)(row - b * t);
  for (int col = lane * 4; col < c; col += 256) {
    const f32x4 g = *reinterpret_cast<const f32x4*>(dout + row * c + col), o = *reinterpret_cast<const f32x4*>(ctx + row * c + col);
    *reinterpret_cast<u32x2*>(dout16 + row * c + col) = u32x2{pack_bf16(g[0], g[1]), pack_bf16(g[2], g[3])};
    float d = (g[0] * o[0] + g[1] * o[1]) + (g[2] * o[2] + g[3] * o[3]);
    d += __shfl_xor(d, 8); d += __shfl_xor(d, 4); d += __shfl_xor(d, 2); d += __shfl_xor(d, 1);
    if ((lane & 15) == 0) dsum[((size_t)b * heads + col / 64) * t + q] = d;
  }
}

// probabilities, mask and dS of one 32-key sub-tile; registers i <-> key kbase + 16 (i / 8) + i % 8, lane <-> one query, wr[16 (i / 8) + i % 8] = the
// bias of (query, key) in natural units, gl = the query's gate in log2 units
//   in:  s = q . k (raw), dp = dO . v (raw);  out: s = P * keep / (1 - p) (the dV operand), dp = dS = P * (dP - D)
__device__ __forceinline__ void wt_bwd_tile(f32x16& s, f32x16& dp, const float* wr, float gl, int kbase, int lim, bool q_ok, float lse2, float dsum,
                                            const WtArgs& a, unsigned long long erow, bool drop) {
  unsigned k_lo = 0xffu, k_hi = 0xffu;
  if (drop) { k_lo = keep8(a.mask, erow + kbase); k_hi = keep8(a.mask, erow + kbase + 16); }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int key = kbase + 16 * (i >> 3) + (i & 7);
    const float z = fmaf(s[i], a.scale_log2e, gl * wr[16 * (i >> 3) + (i & 7)]);
    const float p = (q_ok && key < lim) ? __builtin_amdgcn_exp2f(z - lse2) : 0.f;
    const bool kept = (((i < 8 ? k_lo : k_hi) >> (i & 7)) & 1u) != 0;
    const float ks = kept ? a.keep_scale : 0.f;
    dp[i] = p * (dp[i] * ks - dsum);
    s[i] = p * ks;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// backward, dQ and dg: workgroup = 128 queries of one (clip, head); dQ^T[d][q] += K^T dS^T, dg[q] += sum over the lane's keys of dS rb
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void wt_bwd_dq_kernel(const WtArgs a) {
  __shared__ __attribute__((aligned(16))) char ks_[WT_KT * WT_PITCH];
  __shared__ __attribute__((aligned(16))) char vs_[WT_KT * WT_PITCH];
  __shared__ __attribute__((aligned(16))) float rbs[WT_WIN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, head = blockIdx.y;
  const int qw0 = blockIdx.x * WT_QW, q0 = qw0 + wave * 32;
  const size_t rowp = (size_t)3 * a.c;
  const unsigned short* base = a.qkv + (size_t)b * a.t * rowp + (size_t)head * 64;
  const int lim = wt_lim(a, b);
  const int half = lane >> 5, n32 = lane & 31;
  const int query = q0 + n32;
  const bool q_ok = query < a.t;
  const int qrow = q_ok ? query : a.t - 1;
  const bool drop = a.p_drop > 0.f;
  const size_t bh = (size_t)b * a.heads + head;
  const unsigned long long erow = ((unsigned long long)bh * a.t + qrow) * (unsigned long long)a.t;
  s16x8 qf[4], gf[4];
  {
    const uint4* qp = reinterpret_cast<const uint4*>(base + (size_t)qrow * rowp + 8 * half);
    const uint4* gp = reinterpret_cast<const uint4*>(a.dout + ((size_t)b * a.t + qrow) * a.c + (size_t)head * 64 + 8 * half);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) { qf[ks] = __builtin_bit_cast(s16x8, qp[2 * ks]); gf[ks] = __builtin_bit_cast(s16x8, gp[2 * ks]); }
  }
  const float lse2 = a.lse2[bh * a.t + qrow], dsum = a.dsum[bh * a.t + qrow];
  const float gl = a.gate[bh * a.t + qrow] * LOG2E;
  const float* rbh = a.rb + (size_t)head * (2 * a.t - 1);
  f32x16 dq[2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int i = 0; i < 16; ++i) dq[mt][i] = 0.f;
  float dg = 0.f;
  const int pm = (n32 & ~12) | ((n32 & 4) << 1) | ((n32 & 8) >> 1);
  const int q4 = (lane >> 2) & 3, gq = (lane >> 4) & 1, p4 = lane & 3;
  const int v_off = (8 * half + q4) * WT_PITCH + (16 * gq + 4 * p4) * 2;
  const int wbase = WT_QW - 1 - (wave * 32 + n32) + 8 * half;
  for (int k0 = 0; k0 < lim; k0 += WT_KT) {
    __syncthreads();
    stage_kv(ks_, vs_, base, rowp, a.c, a.t, k0, tid);
    if (tid < WT_WIN) rbs[tid] = rb_at(rbh, a.t, k0 - qw0 - (WT_QW - 1) + tid);
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      if (k0 + sub * 32 >= lim) break;
      f32x16 s, dp;
#pragma unroll
      for (int i = 0; i < 16; ++i) { s[i] = 0.f; dp[i] = 0.f; }
      const char* kr = ks_ + (sub * 32 + pm) * WT_PITCH + half * 16;
      const char* vr = vs_ + (sub * 32 + pm) * WT_PITCH + half * 16;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const s16x8*>(kr + ks * 32), qf[ks], s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const s16x8*>(vr + ks * 32), gf[ks], dp, 0, 0, 0);
      }
      const float* wr = rbs + wbase + 32 * sub;
      wt_bwd_tile(s, dp, wr, gl, k0 + sub * 32 + 8 * half, lim, q_ok, lse2, dsum, a, erow, drop);
#pragma unroll
      for (int i = 0; i < 16; ++i) dg = fmaf(dp[i], wr[16 * (i >> 3) + (i & 7)], dg);
#pragma unroll
      for (int ks2 = 0; ks2 < 2; ++ks2) {
        const unsigned p01 = pack_bf16(dp[8 * ks2 + 0], dp[8 * ks2 + 1]), p23 = pack_bf16(dp[8 * ks2 + 2], dp[8 * ks2 + 3]);
        const unsigned p45 = pack_bf16(dp[8 * ks2 + 4], dp[8 * ks2 + 5]), p67 = pack_bf16(dp[8 * ks2 + 6], dp[8 * ks2 + 7]);
        const s16x8 pb = __builtin_bit_cast(s16x8, uint4{p01, p23, p45, p67});
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
          const char* ka = ks_ + (sub * 32 + 16 * ks2) * WT_PITCH + v_off + 64 * mt;
          const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((TS_LDS s16x4*)((TS_LDS char*)ka));
          const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((TS_LDS s16x4*)((TS_LDS char*)ka + 4 * WT_PITCH));
          const s16x8 kf = s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          dq[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, pb, dq[mt], 0, 0, 0);
        }
      }
    }
  }
  dg += __shfl_xor(dg, 32);
  if (q_ok) {
    float* dst = a.dqkv + ((size_t)b * a.t + query) * rowp + (size_t)head * 64 + 4 * half;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<f32x4*>(dst + 32 * mt + 8 * g) =
            f32x4{dq[mt][4 * g] * a.scale, dq[mt][4 * g + 1] * a.scale, dq[mt][4 * g + 2] * a.scale, dq[mt][4 * g + 3] * a.scale};
    if (half == 0) a.dgate[bh * a.t + query] = dg;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// backward, dK, dV and the drb records: workgroup = 64 keys of one (clip, head), loop over 128-query tiles (32 per wave), as attn_bwd_dkv_kernel;
// each wave also stages the 95 bias diagonals of its 32 x 64 tile, and after the contraction reads its bf16 dS tile back along those diagonals
// (lane l owns diagonals l and l + 64), weighted by the gate of each row: record (clip, head, key tile, query tile)[dd] = sum_q g_q dS[q][q + dd - 31].
// ---------------------------------------------------------------------------------------------------------------------
constexpr int WT_WTILE = 32 * WT_PITCH;       // one [32 rows][64 columns] bf16 tile
constexpr size_t WT_DKV_LDS = (size_t)2 * WT_KT * WT_PITCH + (size_t)4 * 4 * WT_WTILE + (size_t)4 * 96 * sizeof(float);   // 75,264 B

__global__ __launch_bounds__(256) void wt_bwd_dkv_kernel(const WtArgs a) {
  extern __shared__ __attribute__((aligned(16))) char sm[];
  char* const ks_ = sm;
  char* const vs_ = sm + WT_KT * WT_PITCH;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  char* const qt = sm + 2 * WT_KT * WT_PITCH + wave * 4 * WT_WTILE;     // this wave's Q, dO, Pd, dS tiles
  char* const gt = qt + WT_WTILE;
  char* const pt = gt + WT_WTILE;
  char* const st = pt + WT_WTILE;
  float* const rbw = reinterpret_cast<float*>(sm + 2 * WT_KT * WT_PITCH + 4 * 4 * WT_WTILE) + wave * 96;   // this wave's 95 diagonals
  const int b = blockIdx.z, head = blockIdx.y, k0 = blockIdx.x * WT_KT;
  const size_t rowp = (size_t)3 * a.c;
  const unsigned short* base = a.qkv + (size_t)b * a.t * rowp + (size_t)head * 64;
  const int lim = wt_lim(a, b);
  const bool drop = a.p_drop > 0.f;
  const int half = lane >> 5, n32 = lane & 31;
  const size_t bh = (size_t)b * a.heads + head;
  const float* rbh = a.rb + (size_t)head * (2 * a.t - 1);
  const float* gh = a.gate + bh * a.t;
  stage_kv(ks_, vs_, base, rowp, a.c, a.t, k0, tid);
  __syncthreads();
  f32x16 dv[2][2], dk[2][2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int i = 0; i < 16; ++i) { dv[mt][nt][i] = 0.f; dk[mt][nt][i] = 0.f; }
  const int pm = (n32 & ~12) | ((n32 & 4) << 1) | ((n32 & 8) >> 1);
  const int q4 = (lane >> 2) & 3, gq = (lane >> 4) & 1, p4 = lane & 3;
  const int tr_off = (8 * half + q4) * WT_PITCH + (16 * gq + 4 * p4) * 2;
  const int wbase = 31 - n32 + 8 * half;       // window slot of (key k0 + kk, query q0 + qq) is kk - qq + 31
  const bool any_key = k0 < lim;
  float* const rec_base = a.dparts + (bh * a.nkt + blockIdx.x) * (size_t)a.nqt * WT_DG;
  for (int q0 = wave * 32; q0 < a.t && any_key; q0 += WT_QW) {
#pragma unroll
    for (int rep = 0; rep < 4; ++rep) {
      const int chunk = lane + 64 * rep, r = chunk >> 3, cc = chunk & 7;
      const int qr = q0 + r < a.t ? q0 + r : a.t - 1;
      *reinterpret_cast<uint4*>(qt + r * WT_PITCH + cc * 16) = *reinterpret_cast<const uint4*>(base + (size_t)qr * rowp + cc * 8);
      *reinterpret_cast<uint4*>(gt + r * WT_PITCH + cc * 16) = *reinterpret_cast<const uint4*>(a.dout + ((size_t)b * a.t + qr) * a.c + (size_t)head * 64 + cc * 8);
    }
    rbw[lane] = rb_at(rbh, a.t, k0 - q0 - 31 + lane);
    if (lane < WT_DG - 64) rbw[64 + lane] = rb_at(rbh, a.t, k0 - q0 + 33 + lane);
    const int query = q0 + n32;
    const bool q_ok = query < a.t;
    const int qrow = q_ok ? query : a.t - 1;
    const unsigned long long erow = ((unsigned long long)bh * a.t + qrow) * (unsigned long long)a.t;
    const float lse2 = a.lse2[bh * a.t + qrow], dsum = a.dsum[bh * a.t + qrow];
    const float gl = gh[qrow] * LOG2E;
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    s16x8 qf[4], gf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      qf[ks] = *reinterpret_cast<const s16x8*>(qt + n32 * WT_PITCH + (16 * ks + 8 * half) * 2);
      gf[ks] = *reinterpret_cast<const s16x8*>(gt + n32 * WT_PITCH + (16 * ks + 8 * half) * 2);
    }
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      f32x16 s, dp;
#pragma unroll
      for (int i = 0; i < 16; ++i) { s[i] = 0.f; dp[i] = 0.f; }
      const char* kr = ks_ + (sub * 32 + pm) * WT_PITCH + half * 16;
      const char* vr = vs_ + (sub * 32 + pm) * WT_PITCH + half * 16;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const s16x8*>(kr + ks * 32), qf[ks], s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const s16x8*>(vr + ks * 32), gf[ks], dp, 0, 0, 0);
      }
      wt_bwd_tile(s, dp, rbw + wbase + 32 * sub, gl, k0 + sub * 32 + 8 * half, lim, q_ok, lse2, dsum, a, erow, drop);
#pragma unroll
      for (int run = 0; run < 2; ++run) {
        const int col = (32 * sub + 16 * run + 8 * half) * 2;
        *reinterpret_cast<uint4*>(pt + n32 * WT_PITCH + col) = uint4{pack_bf16(s[8 * run + 0], s[8 * run + 1]), pack_bf16(s[8 * run + 2], s[8 * run + 3]),
                                                                      pack_bf16(s[8 * run + 4], s[8 * run + 5]), pack_bf16(s[8 * run + 6], s[8 * run + 7])};
        *reinterpret_cast<uint4*>(st + n32 * WT_PITCH + col) = uint4{pack_bf16(dp[8 * run + 0], dp[8 * run + 1]), pack_bf16(dp[8 * run + 2], dp[8 * run + 3]),
                                                                      pack_bf16(dp[8 * run + 4], dp[8 * run + 5]), pack_bf16(dp[8 * run + 6], dp[8 * run + 7])};
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      s16x8 ga[2], qa[2], pb[2], sb[2];
#pragma unroll
      for (int x = 0; x < 2; ++x) {
        const int off = 16 * ks * WT_PITCH + tr_off + 64 * x;
        auto tr8 = [&](const char* tile) {
          const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((TS_LDS s16x4*)((TS_LDS char*)tile + off));
          const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((TS_LDS s16x4*)((TS_LDS char*)tile + off + 4 * WT_PITCH));
          return s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        };
        ga[x] = tr8(gt); qa[x] = tr8(qt); pb[x] = tr8(pt); sb[x] = tr8(st);
      }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
          dv[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ga[mt], pb[nt], dv[mt][nt], 0, 0, 0);
          dk[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa[mt], sb[nt], dk[mt][nt], 0, 0, 0);
        }
    }
    // ---- the drb record of this (key tile, query tile): diagonal dd <-> key - query = k0 - q0 + dd - 31, rows past t hold dS = 0
    {
      float acc0 = 0.f, acc1 = 0.f;
      const int nq = a.t - q0 < 32 ? a.t - q0 : 32;                            // wave-uniform
      for (int ql = 0; ql < nq; ++ql) {
        const float g = gh[q0 + ql];
        const int kl0 = ql + lane - 31, kl1 = kl0 + 64;
        const TS_LDS unsigned short* row = (const TS_LDS unsigned short*)((TS_LDS char*)st + ql * WT_PITCH);
        if (kl0 >= 0 && kl0 < WT_KT) acc0 = fmaf(g, bf16_to_f32(row[kl0]), acc0);
        if (kl1 < WT_KT) acc1 = fmaf(g, bf16_to_f32(row[kl1]), acc1);
      }
      float* rec = rec_base + (size_t)(q0 >> 5) * WT_DG;
      rec[lane] = acc0;
      if (lane < WT_DG - 64) rec[64 + lane] = acc1;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
  }
  // ---- the four waves' sums (as attn_bwd_dkv_kernel): [wave][mt][nt][16][64 lanes] f32 over the staging area, dv then dk
  __syncthreads();
  float* const red = reinterpret_cast<float*>(sm + 2 * WT_KT * WT_PITCH);
#pragma unroll
  for (int which = 0; which < 2; ++which) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int i = 0; i < 16; ++i) red[(((size_t)wave * 4 + mt * 2 + nt) * 16 + i) * 64 + lane] = which ? dk[mt][nt][i] : dv[mt][nt][i];
    __syncthreads();
    const int mt = wave >> 1, nt = wave & 1;
    f32x16 tot;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      float v = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) v += red[(((size_t)w * 4 + mt * 2 + nt) * 16 + i) * 64 + lane];
      tot[i] = which ? v * a.scale : v;
    }
    const int key = k0 + 32 * nt + n32;
    if (key < a.t) {
      float* dst = a.dqkv + ((size_t)b * a.t + key) * rowp + (size_t)(which ? 1 : 2) * a.c + (size_t)head * 64 + 32 * mt + 4 * half;
#pragma unroll
      for (int g = 0; g < 4; ++g) *reinterpret_cast<f32x4*>(dst + 8 * g) = f32x4{tot[4 * g], tot[4 * g + 1], tot[4 * g + 2], tot[4 * g + 3]};
    }
    __syncthreads();
  }
}

// drb[h][d + t - 1] = sum over clips b, key tiles k0 < key_len[b] and the (at most 3) query tiles q0 whose record holds diagonal d, in that order
__global__ __launch_bounds__(256) void wt_drb_sum_kernel(const float* __restrict__ parts, const int* __restrict__ key_len, int batch, int heads, int t,
                                                         int nkt, int nqt, float* __restrict__ drb) {
  const int h = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  if (j >= 2 * t - 1) return;
  const int d = j - (t - 1);
  float acc = 0.f;
  for (int b = 0; b < batch; ++b) {
    int lim = t;
    if (key_len) lim = key_len[b] < t ? (key_len[b] > 0 ? key_len[b] : 0) : t;
    const float* pb = parts + ((size_t)b * heads + h) * nkt * (size_t)nqt * WT_DG;
    for (int kt = 0; kt < nkt && kt * WT_KT < lim; ++kt) {
      const int k0 = kt * WT_KT;
      const int lo = k0 - d - 31, hi = k0 - d + 63;        // q0 in [lo, hi], a multiple of 32 in [0, t)
      if (hi < 0) continue;
      const int qt_lo = lo <= 0 ? 0 : (lo + 31) >> 5;
      const int qt_hi = (hi >> 5) < nqt - 1 ? (hi >> 5) : nqt - 1;
      for (int q = qt_lo; q <= qt_hi; ++q) acc += pb[((size_t)kt * nqt + q) * WT_DG + (d - k0 + 32 * q + 31)];
    }
  }
  drb[(size_t)h * (2 * t - 1) + j] = acc;
}

// ---------------------------------------------------------------------------------------------------------------------
// gate
// ---------------------------------------------------------------------------------------------------------------------
// one thread per (row n = b t + i, head h): the 8 projections of x[n][64 h .. 64 h + 63]
__global__ __launch_bounds__(256) void wt_gate_fwd_kernel(const float* __restrict__ x, long long ld, const float* __restrict__ w, const float* __restrict__ bias,
                                                          const float* __restrict__ cst, int t, int heads, long long units, float* __restrict__ gate,
                                                          float* __restrict__ gab) {
  __shared__ __attribute__((aligned(16))) float ws[8 * 64];
  ws[threadIdx.x] = w[threadIdx.x];
  ws[256 + threadIdx.x] = w[256 + threadIdx.x];
  __syncthreads();
  const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
  if (u >= units) return;
  const long long n = u / heads;
  const int h = (int)(u - n * heads);
  const long long b = n / t;
  const int i = (int)(n - b * t);
  const float* xr = x + n * ld + 64 * h;
  float p[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) p[r] = 0.f;
#pragma unroll 4
  for (int d = 0; d < 64; d += 4) {
    const f32x4 xv = *reinterpret_cast<const f32x4*>(xr + d);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const f32x4 wv = *reinterpret_cast<const f32x4*>(ws + r * 64 + d);
      p[r] = fmaf(xv[3], wv[3], fmaf(xv[2], wv[2], fmaf(xv[1], wv[1], fmaf(xv[0], wv[0], p[r]))));
    }
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) p[r] += bias[r];
  const float ga = sigmoid_f(((p[0] + p[1]) + p[2]) + p[3]);
  const float gb = sigmoid_f(((p[4] + p[5]) + p[6]) + p[7]);
  const size_t o = ((size_t)b * heads + h) * t + i;
  gate[o] = ga * (gb * cst[h] - 1.f) + 2.f;
  gab[o] = ga;
  gab[(size_t)units + o] = gb;
}

constexpr int WG_ROWS = 256;       // rows per workgroup of the gate backward (64 per wave)
constexpr int WG_REC = 131;        // per-wave partial: 64 sums da x, 64 sums db x, sum da, sum db, sum dg ga gb

// workgroup (row block s, head h), one wave per 64 rows, lane = column d: dx written, per-wave partials of dW / dbeta / dc
__global__ __launch_bounds__(256) void wt_gate_bwd_kernel(const float* __restrict__ x, long long ld, const float* __restrict__ w,
                                                          const float* __restrict__ cst, const float* __restrict__ gab, const float* __restrict__ dgate,
                                                          int t, int heads, long long rows, float* __restrict__ dx, float* __restrict__ parts) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h = blockIdx.y, s = blockIdx.x;
  const float wa = ((w[0 * 64 + lane] + w[1 * 64 + lane]) + w[2 * 64 + lane]) + w[3 * 64 + lane];
  const float wb = ((w[4 * 64 + lane] + w[5 * 64 + lane]) + w[6 * 64 + lane]) + w[7 * 64 + lane];
  const float c = cst[h];
  const size_t units = (size_t)rows * heads;
  float xa = 0.f, xb = 0.f, sa = 0.f, sb = 0.f, sc = 0.f;
  const long long r0 = (long long)s * WG_ROWS + wave * 64;
  for (int r = 0; r < 64 && r0 + r < rows; ++r) {
    const long long n = r0 + r;
    const long long b = n / t;
    const size_t o = ((size_t)b * heads + h) * t + (size_t)(n - b * t);
    const float ga = gab[o], gb = gab[units + o], dg = dgate[o];
    const float da = dg * (gb * c - 1.f) * ga * (1.f - ga);
    const float db = dg * ga * c * gb * (1.f - gb);
    const float xv = x[n * ld + 64 * h + lane];
    xa = fmaf(da, xv, xa);
    xb = fmaf(db, xv, xb);
    sa += da;
    sb += db;
    sc = fmaf(dg, ga * gb, sc);
    dx[n * ld + 64 * h + lane] = fmaf(da, wa, db * wb);
  }
  float* rec = parts + (((size_t)h * gridDim.x + s) * 4 + wave) * WG_REC;
  rec[lane] = xa;
  rec[64 + lane] = xb;
  if (lane == 0) { rec[128] = sa; rec[129] = sb; rec[130] = sc; }
}

// dW [8][64], dbeta [8], dc [H]: one thread per output, the records summed in the order (head, row block, wave)
__global__ __launch_bounds__(256) void wt_gate_sum_kernel(const float* __restrict__ parts, int heads, int blocks, float* __restrict__ dw,
                                                          float* __restrict__ dbias, float* __restrict__ dc) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= 520 + heads) return;
  float acc = 0.f;
  if (o < 520) {
    const int r = o < 512 ? o >> 6 : o - 512;
    const int slot = o < 512 ? (r < 4 ? 0 : 64) + (o & 63) : (r < 4 ? 128 : 129);
    const size_t n = (size_t)heads * blocks * 4;
    for (size_t k = 0; k < n; ++k) acc += parts[k * WG_REC + slot];
    if (o < 512) dw[o] = acc; else dbias[o - 512] = acc;
  } else {
    const int h = o - 520;
    const size_t n = (size_t)blocks * 4;
    for (size_t k = 0; k < n; ++k) acc += parts[((size_t)h * blocks * 4 + k) * WG_REC + 130];
    dc[h] = acc;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// embedding gradient: one wave per (bucket k, head h) gathers the diagonals of bucket k (bucket(d) as wavlm_rel_bias_kernel computes it)
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void wt_rel_bias_bwd_kernel(const float* __restrict__ drb, const int* __restrict__ abs_bucket, int nb, int md, int heads,
                                                              int t, float* __restrict__ dembed) {
  const int lane = threadIdx.x & 63;
  const long long pair = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pair >= (long long)nb * heads) return;
  const int k = (int)(pair / heads), h = (int)(pair - (long long)k * heads);
  const int n = 2 * t - 1;
  const float* row = drb + (size_t)h * n;
  float acc = 0.f;
  for (int j = lane; j < n; j += 64) {
    const int d = j - (t - 1);
    const int ad = d < 0 ? -d : d;
    int bucket = (d > 0 ? nb / 2 : 0) + abs_bucket[ad < md ? ad : md];
    bucket = bucket < 0 ? 0 : (bucket < nb ? bucket : nb - 1);
    if (bucket == k) acc += row[j];
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (lane == 0) dembed[(size_t)k * heads + h] = acc;
}

}  // namespace

}  // namespace ts

using namespace ts;

extern "C" int ts_wavlm_train_abi_version(void) { return TS_WAVLM_TRAIN_ABI_VERSION; }

static int wt_check(const void* qkv, int32_t batch, int32_t t, int32_t c, int32_t heads, float p_drop) {
  if (!qkv || batch <= 0 || t <= 0 || c <= 0 || heads <= 0 || c % heads || !(p_drop >= 0.f && p_drop < 1.f)) return TS_EINVAL;
  if (c / heads != 64 || c % 8 || (reinterpret_cast<uintptr_t>(qkv) & 15) || (long long)batch * heads * t * t >= (1ll << 40)) return TS_EUNSUPPORTED;
  return TS_OK;
}

static int64_t al16(int64_t n) { return (n + 15) / 16 * 16; }
// every element + four words of slack: the dKV kernel reads the 64-bit window of keys up to 62 past the last one
static long long wt_mask_words(int batch, int t, int heads) { return ((long long)batch * heads * t * t + 31) / 32 + 4; }
static void wt_draw_mask(unsigned* mask, int batch, int t, int heads, unsigned long long seed, float p, hipStream_t stream) {
  const long long n = wt_mask_words(batch, t, heads);
  hipLaunchKernelGGL(wt_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, mask, n, seed, p);
}
static int64_t wt_drb_parts(int batch, int t, int heads) {
  return (int64_t)batch * heads * ((t + WT_KT - 1) / WT_KT) * ((t + 31) / 32) * WT_DG;
}

extern "C" int64_t ts_wavlm_attention_train_fwd_workspace(int32_t batch, int32_t t, int32_t c, int32_t heads) {
  if (batch <= 0 || t <= 0 || c <= 0 || heads <= 0) return TS_EINVAL;
  return al16(wt_mask_words(batch, t, heads) * 4);
}

extern "C" int ts_wavlm_attention_train_fwd(const void* qkv_bf16, int32_t batch, int32_t t, int32_t c, int32_t heads, const int32_t* key_len, float p_drop,
                                            uint64_t seed, const float* gate, const float* rel_bias, float* ctx, float* lse2, void* workspace, void* stream_) {
  if (int st = wt_check(qkv_bf16, batch, t, c, heads, p_drop)) return st;
  if (!gate || !rel_bias || !ctx || !lse2 || (p_drop > 0.f && !workspace)) return TS_EINVAL;
  if ((reinterpret_cast<uintptr_t>(ctx) & 15) || (reinterpret_cast<uintptr_t>(workspace) & 15)) return TS_EUNSUPPORTED;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  (void)hipGetLastError();
  if (p_drop > 0.f) wt_draw_mask(static_cast<unsigned*>(workspace), batch, t, heads, seed, p_drop, stream);
  WtArgs a{};
  a.qkv = static_cast<const unsigned short*>(qkv_bf16); a.key_len = key_len; a.gate = gate; a.rb = rel_bias; a.ctx = ctx; a.lse2 = lse2;
  a.t = t; a.c = c; a.heads = heads;
  a.scale = 0.125f; a.scale_log2e = LOG2E * a.scale;
  a.p_drop = p_drop; a.keep_scale = 1.f / (1.f - p_drop);
  a.mask = p_drop > 0.f ? static_cast<const unsigned*>(workspace) : nullptr;
  hipLaunchKernelGGL(wt_fwd_kernel, dim3((t + WT_QW - 1) / WT_QW, heads, batch), dim3(256), 0, stream, a);
  return hip_status(hipGetLastError());
}

// workspace: dO bf16 [B][t][c] | D f32 [B][H][t] | drb records f32 | the mask bits (used when fwd_mask is NULL and p_drop > 0)
extern "C" int64_t ts_wavlm_attention_train_bwd_workspace(int32_t batch, int32_t t, int32_t c, int32_t heads) {
  if (batch <= 0 || t <= 0 || c <= 0 || heads <= 0) return TS_EINVAL;
  return al16((int64_t)batch * t * c * 2) + al16((int64_t)batch * heads * t * 4) + al16(wt_drb_parts(batch, t, heads) * 4) +
         al16(wt_mask_words(batch, t, heads) * 4);
}

extern "C" int ts_wavlm_attention_train_bwd(const void* qkv_bf16, int32_t batch, int32_t t, int32_t c, int32_t heads, const int32_t* key_len, float p_drop,
                                            uint64_t seed, const float* gate, const float* rel_bias, const float* dctx, const float* ctx, const float* lse2,
                                            const void* fwd_mask, float* dqkv, float* dgate, float* drel_bias, void* workspace, void* stream_) {
  if (int st = wt_check(qkv_bf16, batch, t, c, heads, p_drop)) return st;
  if (!gate || !rel_bias || !dctx || !ctx || !lse2 || !dqkv || !dgate || !drel_bias || !workspace) return TS_EINVAL;
  if ((reinterpret_cast<uintptr_t>(dctx) & 15) || (reinterpret_cast<uintptr_t>(ctx) & 15) || (reinterpret_cast<uintptr_t>(dqkv) & 15) ||
      (reinterpret_cast<uintptr_t>(workspace) & 15))
    return TS_EUNSUPPORTED;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  char* wsp = static_cast<char*>(workspace);
  unsigned short* const dout16 = reinterpret_cast<unsigned short*>(wsp);
  wsp += al16((int64_t)batch * t * c * 2);
  float* const dsum = reinterpret_cast<float*>(wsp);
  wsp += al16((int64_t)batch * heads * t * 4);
  float* const parts = reinterpret_cast<float*>(wsp);
  wsp += al16(wt_drb_parts(batch, t, heads) * 4);
  WtArgs a{};
  a.qkv = static_cast<const unsigned short*>(qkv_bf16); a.key_len = key_len; a.gate = gate; a.rb = rel_bias;
  a.lse2 = const_cast<float*>(lse2); a.dout = dout16; a.dsum = dsum; a.dqkv = dqkv; a.dgate = dgate; a.dparts = parts;
  a.t = t; a.c = c; a.heads = heads; a.nkt = (t + WT_KT - 1) / WT_KT; a.nqt = (t + 31) / 32;
  a.scale = 0.125f; a.scale_log2e = LOG2E * a.scale;
  a.p_drop = p_drop; a.keep_scale = 1.f / (1.f - p_drop);
  (void)hipGetLastError();
  if (p_drop > 0.f && fwd_mask) a.mask = static_cast<const unsigned*>(fwd_mask);
  else if (p_drop > 0.f) {
    unsigned* const mask = reinterpret_cast<unsigned*>(wsp);
    wt_draw_mask(mask, batch, t, heads, seed, p_drop, stream);
    a.mask = mask;
  }
  const long long rows = (long long)batch * t;
  hipLaunchKernelGGL(wt_rowdot_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, dctx, ctx, dout16, dsum, rows, t, c, heads);
  hipLaunchKernelGGL(wt_bwd_dq_kernel, dim3((t + WT_QW - 1) / WT_QW, heads, batch), dim3(256), 0, stream, a);
  static bool attr[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return TS_EINVAL;
  if (!attr[dev]) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(wt_bwd_dkv_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)WT_DKV_LDS) != hipSuccess)
      return TS_EUNSUPPORTED;
    attr[dev] = true;
  }
  hipLaunchKernelGGL(wt_bwd_dkv_kernel, dim3(a.nkt, heads, batch), dim3(256), WT_DKV_LDS, stream, a);
  hipLaunchKernelGGL(wt_drb_sum_kernel, dim3((unsigned)((2 * t - 1 + 255) / 256), heads), dim3(256), 0, stream, parts, key_len, batch, heads, t, a.nkt,
                     a.nqt, drel_bias);
  return hip_status(hipGetLastError());
}

extern "C" int ts_wavlm_gate_fwd(const float* x, int32_t batch, int32_t t, int32_t heads, int64_t ld_x, const float* gate_w, const float* gate_b,
                                 const float* gate_const, float* gate, float* gate_ab, void* stream_) {
  if (!x || !gate_w || !gate_b || !gate_const || !gate || !gate_ab || batch <= 0 || t <= 0 || heads <= 0 || ld_x < 64LL * heads) return TS_EINVAL;
  if (ld_x % 4 || (reinterpret_cast<uintptr_t>(x) & 15)) return TS_EUNSUPPORTED;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  (void)hipGetLastError();
  const long long units = (long long)batch * t * heads;
  hipLaunchKernelGGL(wt_gate_fwd_kernel, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, stream, x, (long long)ld_x, gate_w, gate_b, gate_const, t, heads,
                     units, gate, gate_ab);
  return hip_status(hipGetLastError());
}

static int wt_gate_blocks(int batch, int t) { return (int)(((long long)batch * t + WG_ROWS - 1) / WG_ROWS); }

extern "C" int64_t ts_wavlm_gate_bwd_workspace(int32_t batch, int32_t t, int32_t heads) {
  if (batch <= 0 || t <= 0 || heads <= 0) return TS_EINVAL;
  return al16((int64_t)heads * wt_gate_blocks(batch, t) * 4 * WG_REC * 4);
}

extern "C" int ts_wavlm_gate_bwd(const float* x, int32_t batch, int32_t t, int32_t heads, int64_t ld_x, const float* gate_w, const float* gate_const,
                                 const float* gate_ab, const float* dgate, float* dx, float* dgate_w, float* dgate_b, float* dgate_const, void* workspace,
                                 void* stream_) {
  if (!x || !gate_w || !gate_const || !gate_ab || !dgate || !dx || !dgate_w || !dgate_b || !dgate_const || !workspace || batch <= 0 || t <= 0 ||
      heads <= 0 || ld_x < 64LL * heads)
    return TS_EINVAL;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  (void)hipGetLastError();
  const int blocks = wt_gate_blocks(batch, t);
  float* const parts = static_cast<float*>(workspace);
  hipLaunchKernelGGL(wt_gate_bwd_kernel, dim3(blocks, heads), dim3(256), 0, stream, x, (long long)ld_x, gate_w, gate_const, gate_ab, dgate, t, heads,
                     (long long)batch * t, dx, parts);
  hipLaunchKernelGGL(wt_gate_sum_kernel, dim3((unsigned)((520 + heads + 255) / 256)), dim3(256), 0, stream, parts, heads, blocks, dgate_w, dgate_b,
                     dgate_const);
  return hip_status(hipGetLastError());
}

extern "C" int ts_wavlm_rel_bias_bwd(const float* drel_bias, const int32_t* abs_bucket, int32_t num_buckets, int32_t max_distance, int32_t heads,
                                     int32_t t, float* dembed, void* stream_) {
  if (!drel_bias || !abs_bucket || !dembed || num_buckets < 2 || max_distance < 0 || heads <= 0 || t <= 0) return TS_EINVAL;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  (void)hipGetLastError();
  const long long pairs = (long long)num_buckets * heads;
  hipLaunchKernelGGL(wt_rel_bias_bwd_kernel, dim3((unsigned)((pairs + 3) / 4)), dim3(256), 0, stream, drel_bias, abs_bucket, num_buckets, max_distance,
                     heads, t, dembed);
  return hip_status(hipGetLastError());
}
