// Mixed-precision WavLM FINE-TUNING: the gated relative-position attention of transformers' WavLMAttention (modeling_wavlm.py forward /
// compute_bias, reached through huggingface/compatibility.py:31-42 under the reference's training_step, module.py:102-127) forward and backward
// without the [T][T] matrices, plus the gate and the position-bias embedding with their gradients.  Declared in
// include/thunder_speech_amd/wavlm_train.h.  The attention kernels are the sequences of csrc/attn_tile.hpp with the bias pieces of its WavLM
// section; the mask kernel, the row-dot kernel and the argument check are those of csrc/w2v_attn_train.hip (the wav2vec2 path):
//
//   ts_wavlm_gate_fwd       g[b][h][i] = ga (gb c_h - 1) + 2, ga = sigmoid(p0..3), gb = sigmoid(p4..7), p = x_h W^T + beta   (ga, gb kept)
//   ts_wavlm_gate_bwd       dp0..3 = dg (gb c - 1) ga (1 - ga), dp4..7 = dg ga c gb (1 - gb): dx_h = dp W (written), dW / dbeta / dc from per-wave
//                           partials summed in a fixed order (wavlm_gate_sum_kernel)
//   ts_wavlm_attention_train_fwd   attn_fwd_train_kernel + the bias of wavlm_flash_attn_kernel: the logit s q.k + g[i] rb[j - i + t - 1] (log2
//                           units) formed before the running maximum, the tile's diagonals staged in LDS; ctx f32 and lse2 (bias included)
//   ts_wavlm_attention_train_bwd   attn_rowdot_kernel, then the dQ and dKV sequences rebuilding P with the bias (bwd_tile<true>), and
//                           dg[b][h][i] = sum_j dS_ij rb[j - i + t - 1]          (dQ kernel: the lane owns query i)
//                           drb[h][d + t - 1] = sum_b sum_i g_i dS[i][i + d]      (dKV kernel: the wave's bf16 dS tile [32 q][64 k] read back along
//                           its 95 diagonals, one record per (clip, head, key tile, 32-query tile); wavlm_drb_sum_kernel adds the records of a
//                           diagonal in a fixed order)
//   ts_wavlm_rel_bias_bwd   dE[k][h] = sum over the diagonals d with bucket(d) = k of drb[h][d + t - 1]: one wave per (bucket, head), a gather
// No float atomics anywhere: two calls give the same bits.
#include "attn_tile.hpp"
#include "thunder_speech_amd/wavlm_train.h"

namespace ts {

namespace {

constexpr int WT_DG = 95;          // diagonals of a 32 x 64 tile: the dKV kernel's per-wave window and drb record

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
  const unsigned* mask;            // keep bits of the [B H T][T] dropout stream (attn_mask_kernel); NULL when p_drop == 0
};

// ---------------------------------------------------------------------------------------------------------------------
// forward: attn_fwd_train_kernel with the gated bias in the logit
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void wt_fwd_kernel(const WtArgs a) {
  __shared__ __attribute__((aligned(16))) char ks_[AT_KV];
  __shared__ __attribute__((aligned(16))) char vs_[AT_KV];
  __shared__ __attribute__((aligned(16))) float rbs[AT_WIN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, head = blockIdx.y;
  const int qw0 = blockIdx.x * AT_QW, q0 = qw0 + wave * 32;
  const size_t rowp = (size_t)3 * a.c;
  const unsigned short* base = a.qkv + (size_t)b * a.t * rowp + (size_t)head * 64;
  const int lim = key_limit<false>(a.key_len, b, a.t);
  const TileLane g = tile_lane(lane);
  const int query = q0 + g.n32;
  const int qrow = query < a.t ? query : a.t - 1;
  const bool drop = a.p_drop > 0.f;
  const size_t bh = (size_t)b * a.heads + head;
  const unsigned long long erow = ((unsigned long long)bh * a.t + qrow) * (unsigned long long)a.t;
  s16x8 qf[4];
  load_row_frags(qf, base + (size_t)qrow * rowp + 8 * g.half);
  const float gl = a.gate[bh * a.t + qrow] * LOG2E;
  const float* rbh = a.rb + (size_t)head * (2 * a.t - 1);
  f32x16 o[2];
  zero(o[0]); zero(o[1]);
  float m_run = -INFINITY, l_run = 0.f;
  const int wbase = window_base(wave, g);

  for (int k0 = 0; k0 < lim; k0 += AT_KT) {
    __syncthreads();
    stage_kv(ks_, vs_, base, rowp, a.c, a.t, k0, tid);
    stage_window(rbs, rbh, a.t, k0, qw0, tid);
    __syncthreads();
    const bool full = k0 + AT_KT <= lim;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      if (k0 + sub * 32 >= lim) break;
      f32x16 s = wavlm_logits(qk_subtile(ks_, sub, g, qf), a.scale_log2e, gl, rbs + wbase + 32 * sub);
      const int kbase = k0 + sub * 32 + 8 * g.half;
      if (!full) s = mask_tail(s, kbase, lim);
      const SoftmaxStep sm = softmax_step<false>(s, m_run, l_run);
      m_run = sm.m; l_run = sm.l;
      const f32x16 p = drop ? drop_keys(sm.p, a.mask, erow + kbase, a.keep_scale) : sm.p;
      rescale(o, sm.alpha);
      acc_tile_t(o, p, vs_, sub, g);
    }
  }
  const float l = l_run + __shfl_xor(l_run, 32);
  const float inv = l > 0.f ? 1.f / l : 0.f;
  if (query < a.t) {
    store_f32(a.ctx + ((size_t)b * a.t + query) * a.c + (size_t)head * 64 + 4 * g.half, o, inv);
    if (g.half == 0) a.lse2[bh * a.t + query] = l > 0.f ? m_run + __builtin_amdgcn_logf(l) : INFINITY;      // v_log_f32 = log2
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// backward, dQ and dg: attn_bwd_dq_kernel with the bias, and dg[q] += sum over the lane's keys of dS rb
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void wt_bwd_dq_kernel(const WtArgs a) {
  __shared__ __attribute__((aligned(16))) char ks_[AT_KV];
  __shared__ __attribute__((aligned(16))) char vs_[AT_KV];
  __shared__ __attribute__((aligned(16))) float rbs[AT_WIN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, head = blockIdx.y;
  const int qw0 = blockIdx.x * AT_QW, q0 = qw0 + wave * 32;
  const size_t rowp = (size_t)3 * a.c;
  const unsigned short* base = a.qkv + (size_t)b * a.t * rowp + (size_t)head * 64;
  const int lim = key_limit<false>(a.key_len, b, a.t);
  const TileLane g = tile_lane(lane);
  const int query = q0 + g.n32;
  const bool q_ok = query < a.t;
  const int qrow = q_ok ? query : a.t - 1;
  const bool drop = a.p_drop > 0.f;
  const size_t bh = (size_t)b * a.heads + head;
  const unsigned long long erow = ((unsigned long long)bh * a.t + qrow) * (unsigned long long)a.t;
  s16x8 qf[4], gf[4];
  load_row_frags(qf, base + (size_t)qrow * rowp + 8 * g.half);
  load_row_frags(gf, a.dout + ((size_t)b * a.t + qrow) * a.c + (size_t)head * 64 + 8 * g.half);
  const float lse2 = a.lse2[bh * a.t + qrow], dsum = a.dsum[bh * a.t + qrow];
  const float gl = a.gate[bh * a.t + qrow] * LOG2E;
  const float* rbh = a.rb + (size_t)head * (2 * a.t - 1);
  f32x16 dq[2];
  zero(dq[0]); zero(dq[1]);
  float dg = 0.f;
  const int wbase = window_base(wave, g);
  for (int k0 = 0; k0 < lim; k0 += AT_KT) {
    __syncthreads();
    stage_kv(ks_, vs_, base, rowp, a.c, a.t, k0, tid);
    stage_window(rbs, rbh, a.t, k0, qw0, tid);
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      if (k0 + sub * 32 >= lim) break;
      f32x16 s, dp;
      qk_dp_subtile(s, dp, ks_, vs_, sub, g, qf, gf);
      const float* wr = rbs + wbase + 32 * sub;
      bwd_tile<true>(s, dp, k0 + sub * 32 + 8 * g.half, lim, q_ok, lse2, dsum, a.scale_log2e, a.keep_scale, a.mask, erow, drop, wr, gl);
#pragma unroll
      for (int i = 0; i < 16; ++i) dg = fmaf(dp[i], wr[16 * (i >> 3) + (i & 7)], dg);
      acc_tile_t(dq, dp, ks_, sub, g);
    }
  }
  dg += __shfl_xor(dg, 32);
  if (q_ok) {
    store_f32(a.dqkv + ((size_t)b * a.t + query) * rowp + (size_t)head * 64 + 4 * g.half, dq, a.scale);
    if (g.half == 0) a.dgate[bh * a.t + query] = dg;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// backward, dK, dV and the drb records: attn_bwd_dkv_kernel with the bias; each wave also stages the 95 bias diagonals of its 32 x 64 tile, and after
// the contraction reads its bf16 dS tile back along those diagonals (lane l owns diagonals l and l + 64), weighted by the gate of each row:
// record (clip, head, key tile, query tile)[dd] = sum_q g_q dS[q][q + dd - 31].
// ---------------------------------------------------------------------------------------------------------------------
constexpr size_t WT_DKV_LDS = AT_DKV_LDS + (size_t)4 * 96 * sizeof(float);   // 75,264 B

__global__ __launch_bounds__(256) void wt_bwd_dkv_kernel(const WtArgs a) {
  extern __shared__ __attribute__((aligned(16))) char sm[];
  char* const ks_ = sm;
  char* const vs_ = sm + AT_KV;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  char* const wt = sm + 2 * AT_KV + wave * 4 * AT_WTILE;     // this wave's Q, dO, Pd, dS tiles
  char* const st = wt + 3 * AT_WTILE;
  float* const rbw = reinterpret_cast<float*>(sm + AT_DKV_LDS) + wave * 96;   // this wave's 95 diagonals
  const int b = blockIdx.z, head = blockIdx.y, k0 = blockIdx.x * AT_KT;
  const size_t rowp = (size_t)3 * a.c;
  const unsigned short* base = a.qkv + (size_t)b * a.t * rowp + (size_t)head * 64;
  const int lim = key_limit<false>(a.key_len, b, a.t);
  const bool drop = a.p_drop > 0.f;
  const TileLane g = tile_lane(lane);
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
  const int wbase = 31 - g.n32 + 8 * g.half;       // window slot of (key k0 + kk, query q0 + qq) is kk - qq + 31
  const bool any_key = k0 < lim;
  float* const rec_base = a.dparts + (bh * a.nkt + blockIdx.x) * (size_t)a.nqt * WT_DG;
  for (int q0 = wave * 32; q0 < a.t && any_key; q0 += AT_QW) {
    dkv_stage_rows(wt, base, rowp, a.dout, b, head, a.t, a.c, q0, lane);
    rbw[lane] = rb_at(rbh, a.t, k0 - q0 - 31 + lane);
    if (lane < WT_DG - 64) rbw[64 + lane] = rb_at(rbh, a.t, k0 - q0 + 33 + lane);
    const int query = q0 + g.n32;
    const bool q_ok = query < a.t;
    const int qrow = q_ok ? query : a.t - 1;
    const unsigned long long erow = ((unsigned long long)bh * a.t + qrow) * (unsigned long long)a.t;
    const float lse2 = a.lse2[bh * a.t + qrow], dsum = a.dsum[bh * a.t + qrow];
    const float gl = gh[qrow] * LOG2E;
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    s16x8 qf[4], gf[4];
    dkv_load_frags(qf, gf, wt, g);
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      f32x16 s, dp;
      qk_dp_subtile(s, dp, ks_, vs_, sub, g, qf, gf);
      bwd_tile<true>(s, dp, k0 + sub * 32 + 8 * g.half, lim, q_ok, lse2, dsum, a.scale_log2e, a.keep_scale, a.mask, erow, drop, rbw + wbase + 32 * sub, gl);
      dkv_store_tiles(wt, s, dp, sub, g);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      s16x8 ga[2], qa[2], pb[2], sb[2];
      dkv_operands(ga, qa, pb, sb, wt, ks, g, g.tr_off);
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
        const float gq = gh[q0 + ql];
        const int kl0 = ql + lane - 31, kl1 = kl0 + 64;
        const TS_LDS unsigned short* row = (const TS_LDS unsigned short*)((TS_LDS char*)st + ql * AT_PITCH);
        if (kl0 >= 0 && kl0 < AT_KT) acc0 = fmaf(gq, bf16_to_f32(row[kl0]), acc0);
        if (kl1 < AT_KT) acc1 = fmaf(gq, bf16_to_f32(row[kl1]), acc1);
      }
      float* rec = rec_base + (size_t)(q0 >> 5) * WT_DG;
      rec[lane] = acc0;
      if (lane < WT_DG - 64) rec[64 + lane] = acc1;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  dkv_reduce_store(reinterpret_cast<float*>(sm + 2 * AT_KV), dv, dk, a.scale, a.dqkv, rowp, b, a.t, a.c, head, k0, wave, lane, g);
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
    for (int kt = 0; kt < nkt && kt * AT_KT < lim; ++kt) {
      const int k0 = kt * AT_KT;
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
// embedding gradient: one wave per (bucket k, head h) gathers the diagonals of bucket k
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
    if (wavlm_bucket(j - (t - 1), nb, md, abs_bucket) == k) acc += row[j];
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (lane == 0) dembed[(size_t)k * heads + h] = acc;
}

}  // namespace

}  // namespace ts

using namespace ts;

extern "C" int ts_wavlm_train_abi_version(void) { return TS_WAVLM_TRAIN_ABI_VERSION; }

static int64_t wt_drb_parts(int batch, int t, int heads) {
  return (int64_t)batch * heads * ((t + AT_KT - 1) / AT_KT) * ((t + 31) / 32) * WT_DG;
}

extern "C" int64_t ts_wavlm_attention_train_fwd_workspace(int32_t batch, int32_t t, int32_t c, int32_t heads) {
  if (batch <= 0 || t <= 0 || c <= 0 || heads <= 0) return TS_EINVAL;
  return al16(attn_mask_words(batch, t, heads) * 4);
}

extern "C" int ts_wavlm_attention_train_fwd(const void* qkv_bf16, int32_t batch, int32_t t, int32_t c, int32_t heads, const int32_t* key_len, float p_drop,
                                            uint64_t seed, const float* gate, const float* rel_bias, float* ctx, float* lse2, void* workspace, void* stream_) {
  if (int st = attn_train_check(qkv_bf16, batch, t, c, heads, p_drop)) return st;
  if (!gate || !rel_bias || !ctx || !lse2 || (p_drop > 0.f && !workspace)) return TS_EINVAL;
  if ((reinterpret_cast<uintptr_t>(ctx) & 15) || (reinterpret_cast<uintptr_t>(workspace) & 15)) return TS_EUNSUPPORTED;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  (void)hipGetLastError();
  if (p_drop > 0.f) attn_draw_mask(static_cast<unsigned*>(workspace), batch, t, heads, seed, p_drop, stream);
  WtArgs a{};
  a.qkv = static_cast<const unsigned short*>(qkv_bf16); a.key_len = key_len; a.gate = gate; a.rb = rel_bias; a.ctx = ctx; a.lse2 = lse2;
  a.t = t; a.c = c; a.heads = heads;
  a.scale = 0.125f; a.scale_log2e = LOG2E * a.scale;
  a.p_drop = p_drop; a.keep_scale = 1.f / (1.f - p_drop);
  a.mask = p_drop > 0.f ? static_cast<const unsigned*>(workspace) : nullptr;
  hipLaunchKernelGGL(wt_fwd_kernel, dim3((t + AT_QW - 1) / AT_QW, heads, batch), dim3(256), 0, stream, a);
  return hip_status(hipGetLastError());
}

// workspace: dO bf16 [B][t][c] | D f32 [B][H][t] | drb records f32 | the mask bits (used when fwd_mask is NULL and p_drop > 0)
extern "C" int64_t ts_wavlm_attention_train_bwd_workspace(int32_t batch, int32_t t, int32_t c, int32_t heads) {
  if (batch <= 0 || t <= 0 || c <= 0 || heads <= 0) return TS_EINVAL;
  return al16((int64_t)batch * t * c * 2) + al16((int64_t)batch * heads * t * 4) + al16(wt_drb_parts(batch, t, heads) * 4) +
         al16(attn_mask_words(batch, t, heads) * 4);
}

extern "C" int ts_wavlm_attention_train_bwd(const void* qkv_bf16, int32_t batch, int32_t t, int32_t c, int32_t heads, const int32_t* key_len, float p_drop,
                                            uint64_t seed, const float* gate, const float* rel_bias, const float* dctx, const float* ctx, const float* lse2,
                                            const void* fwd_mask, float* dqkv, float* dgate, float* drel_bias, void* workspace, void* stream_) {
  if (int st = attn_train_check(qkv_bf16, batch, t, c, heads, p_drop)) return st;
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
  a.t = t; a.c = c; a.heads = heads; a.nkt = (t + AT_KT - 1) / AT_KT; a.nqt = (t + 31) / 32;
  a.scale = 0.125f; a.scale_log2e = LOG2E * a.scale;
  a.p_drop = p_drop; a.keep_scale = 1.f / (1.f - p_drop);
  (void)hipGetLastError();
  if (p_drop > 0.f && fwd_mask) a.mask = static_cast<const unsigned*>(fwd_mask);
  else if (p_drop > 0.f) {
    unsigned* const mask = reinterpret_cast<unsigned*>(wsp);
    attn_draw_mask(mask, batch, t, heads, seed, p_drop, stream);
    a.mask = mask;
  }
  attn_rowdot(dctx, ctx, dout16, dsum, batch, t, c, heads, stream);
  hipLaunchKernelGGL(wt_bwd_dq_kernel, dim3((t + AT_QW - 1) / AT_QW, heads, batch), dim3(256), 0, stream, a);
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
