// Fused self-attention for mixed-precision wav2vec2 FINE-TUNING, head_dim 64 (ts_w2v_attention_train_*, below) and head_dim 80 (XLS-R 1B / MMS: hidden
// 1280, 16 heads; ts_mms_attention_train_*, csrc/mms_train.hip): forward and backward without the [T][T] score / probability
// matrices of the unfused path (huggingface/train.py Attention: 127 MB of f32 per layer at 8 x 10 s, written and re-read by six products, two
// softmax passes and two dropout passes -- 28 of the step's 58 ms, profiles/round6_c5_finetune.md).  The reference reaches this code through
// transformers' Wav2Vec2Attention inside AutoModelForCTC (thunder huggingface/compatibility.py:31-42) under Lightning's training_step
// (module.py:102-127): ctx = dropout(softmax(q k^T / sqrt(hd) + key mask)) v.
//
//   forward   (attn_fwd_train_kernel)  the base sequence of csrc/attn_tile.hpp (S^T = K Q^T on v_mfma_f32_32x32x16_bf16, online softmax with a lane
//             owning one query column, O^T += V^T P^T with P^T straight out of the accumulators) + the dropout mask of ts_train_dropout
//             (Philox4x32-10, element e = ((b H + h) T + q) T + k -> word e & 3 of block e >> 2; attn_mask_kernel) + the row statistic
//             lse2 = max + log2(sum) (log2 domain, scale folded in) that lets the backward rebuild any probability as exp2(s c - lse2);
//   backward  two kernels, each recomputing the probabilities and the mask (no atomics, fixed summation order):
//             attn_bwd_dq_kernel    workgroup = 128 queries, loop over key tiles:   dQ^T[d][q] += K^T dS^T   (the forward's second product with K, dS)
//             attn_bwd_dkv_kernel   workgroup = 64 keys, loop over query tiles:     dV += Pd^T dO,  dK += dS^T Q   (P / dS tiles through wave-private LDS)
//             with dP = (dO V^T) * keep / (1 - p),  dS = P * (dP - D),  D[q] = sum_d dO[q][d] O[q][d]  (attn_rowdot_kernel at head_dim 64,
//             attn_rowdot80_kernel at 80, which also cast dO).
// Operands bf16 (q, k, v, dO, P, dS), accumulation and softmax arithmetic f32, results f32 (ctx, dqkv).
// The three attention kernels are templates on the head dimension; the geometry of each instantiation (k-steps, d blocks, LDS pitches) is AttnGeom<HD>
// of csrc/attn_tile.hpp.  The tiles are 64 keys x 32-key sub-tiles at either head dimension, so the mask's slack words cover both.
// The mask kernel, the head_dim 64 row-dot kernel, the argument check and the mask-word count serve the WavLM path (csrc/wavlm_train.hip) too: it
// reaches them through the host functions declared in csrc/attn_tile.hpp.
#include "attn_tile.hpp"
#include "ts_philox.hpp"

namespace ts {

namespace {

struct TaArgs {
  const unsigned short* qkv;       // [B][T][3C] bf16
  const int* key_len;
  float* ctx;                      // forward: [B][T][C] f32
  float* lse2;                     // [B][H][T]
  const unsigned short* dout;      // backward: [B][T][C] bf16
  const float* dsum;               // backward: D [B][H][T]
  float* dqkv;                     // backward: [B][T][3C] f32
  int t, c, heads;
  float scale_log2e, scale;        // log2(e) / sqrt(hd), 1 / sqrt(hd)
  float p_drop, keep_scale;        // dropout probability, 1 / (1 - p)
  const unsigned* mask;            // keep bits of the whole [B H T][T] dropout stream, bit e of the flat bitstring (attn_mask_kernel); NULL when p_drop == 0
};

// The dropout mask as a bitstring, drawn ONCE per call by its own small kernel: bit e is set iff element e of the logical [B * heads * T][T] probability
// matrix keeps its value -- ts_train_dropout's rule: u01(word e & 3 of Philox block e >> 2) >= p.  A thread draws the 8 blocks of one 32-bit word.  Drawing
// the mask inside the attention kernels cost three Philox blocks per 8 probabilities (T is odd: a lane's run of 8 keys straddles three blocks) in each of the
// three kernels -- more than the attention arithmetic itself; now they read two words per run.
__global__ __launch_bounds__(256) void attn_mask_kernel(unsigned* __restrict__ mask, long long n_words, unsigned long long seed, float p) {
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

// ---------------------------------------------------------------------------------------------------------------------
// forward.  amdgpu_waves_per_eu (AttnGeom<HD>::FWD_TRAIN_WAVES): the loop is bound by the softmax's quarter-rate exp2, which only other resident waves
// hide, so head_dim 64 takes the budget of 4 waves that the inference kernels take.  At head_dim 80 that budget leaves this kernel (which also carries the
// dropout row index and the mask pointer) 7 spilled VGPRs with one reload inside the key loop; at 3 the compiler reports 151 VGPRs and no scratch.
// All four head_dim 80 kernels' reports: profiles/xlsr1b_finetune.md.
// ---------------------------------------------------------------------------------------------------------------------
template <int HD>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(AttnGeom<HD>::FWD_TRAIN_WAVES, AttnGeom<HD>::FWD_TRAIN_WAVES))) void attn_fwd_train_kernel(
    const TaArgs a) {
  using G = AttnGeom<HD>;
  __shared__ __attribute__((aligned(16))) char ks_[AT_KT * G::RP];
  __shared__ __attribute__((aligned(16))) char vs_[AT_KT * G::TP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, head = blockIdx.y;
  const int q0 = blockIdx.x * AT_QW + wave * 32;
  const size_t rowp = (size_t)3 * a.c;
  const unsigned short* base = a.qkv + (size_t)b * a.t * rowp + (size_t)head * HD;
  const int lim = key_limit<false>(a.key_len, b, a.t);
  const TileLane g = tile_lane<G::TP>(lane);
  const int query = q0 + g.n32;
  const int qrow = query < a.t ? query : a.t - 1;
  const bool drop = a.p_drop > 0.f;
  const unsigned long long erow = mask_row(b, a.heads, head, a.t, qrow);
  zero_pad<HD, G::TP>(vs_, AT_KT, tid, 256);                                  // the loop's first barrier orders it before any read
  s16x8 qf[HD / 16];
  load_row_frags(qf, base + (size_t)qrow * rowp + 8 * g.half);
  f32x16 o[(HD + 31) / 32];
#pragma unroll
  for (int mt = 0; mt < (HD + 31) / 32; ++mt) zero(o[mt]);
  float m_run = -INFINITY, l_run = 0.f;

  for (int k0 = 0; k0 < lim; k0 += AT_KT) {
    __syncthreads();                                                          // the previous tile has been consumed
    stage_kv<HD, G::RP, G::TP>(ks_, vs_, base, rowp, a.c, a.t, k0, tid);
    __syncthreads();
    const bool full = k0 + AT_KT <= lim;                                      // no masked key in this tile (uniform)
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      if (k0 + sub * 32 >= lim) break;                                        // uniform: nothing but masked keys
      f32x16 s = qk_subtile<G::RP>(ks_, sub, g, qf);
      const int kbase = k0 + sub * 32 + 8 * g.half;
      if (!full) s = mask_tail(s, kbase, lim);
      const SoftmaxStep sm = softmax_step<true>(s, m_run, l_run, a.scale_log2e);
      m_run = sm.m; l_run = sm.l;
      const f32x16 p = drop ? drop_keys(sm.p, a.mask, erow + kbase, a.keep_scale) : sm.p;
      rescale(o, sm.alpha);
      acc_tile_t<G::TP>(o, p, vs_, sub, g);
    }
  }
  const float l = l_run + __shfl_xor(l_run, 32);
  const float inv = l > 0.f ? 1.f / l : 0.f;     // (no valid key: zeros, and a row statistic that makes every rebuilt probability 0)
  if (query < a.t) {
    store_f32<HD>(a.ctx + ((size_t)b * a.t + query) * a.c + (size_t)head * HD + 4 * g.half, o, inv);
    if (g.half == 0) a.lse2[((size_t)b * a.heads + head) * a.t + query] = l > 0.f ? m_run + __builtin_amdgcn_logf(l) : INFINITY;      // v_log_f32 = log2
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// backward, part 0: bf16 copy of dO and D[b][h][q] = sum_d dO[q][d] O[q][d] over the head's columns.  Two kernels, because their summation orders differ and
// the bits of D follow the order.  Head_dim 64: one wave per (b, q) row, four columns per lane, four exchanges over 16 lanes.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attn_rowdot_kernel(const float* __restrict__ dout, const float* __restrict__ ctx, unsigned short* __restrict__ dout16,
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

// Head_dim 80: four lanes per (b, q, head): lane j of the four takes columns 16 i + 4 j .. + 3 for i = 0 .. 4 (a quad reads 64 consecutive bytes per
// step), then two exchanges inside the quad.
__global__ __launch_bounds__(256) void attn_rowdot80_kernel(const float* __restrict__ dout, const float* __restrict__ ctx, unsigned short* __restrict__ dout16,
                                                            float* __restrict__ dsum, long long units, int t, int c, int heads) {
  const long long unit = (long long)blockIdx.x * 64 + (threadIdx.x >> 2);      // (b t + q) heads + h
  if (unit >= units) return;                                                   // whole quads leave together
  const int j = threadIdx.x & 3;
  const long long row = unit / heads;
  const int h = (int)(unit - row * heads);
  const long long b = row / t;
  const int q = (int)(row - b * t);
  const size_t off = (size_t)row * c + (size_t)h * 80 + 4 * j;
  float d = 0.f;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const f32x4 gv = *reinterpret_cast<const f32x4*>(dout + off + 16 * i), ov = *reinterpret_cast<const f32x4*>(ctx + off + 16 * i);
    *reinterpret_cast<u32x2*>(dout16 + off + 16 * i) = u32x2{pack_bf16(gv[0], gv[1]), pack_bf16(gv[2], gv[3])};
    d += (gv[0] * ov[0] + gv[1] * ov[1]) + (gv[2] * ov[2] + gv[3] * ov[3]);
  }
  d += __shfl_xor(d, 2); d += __shfl_xor(d, 1);
  if (j == 0) dsum[((size_t)b * heads + h) * t + q] = d;
}

// ---------------------------------------------------------------------------------------------------------------------
// backward, dQ: workgroup = 128 queries of one (clip, head); K / V tiles of 64 keys through LDS; dQ^T[d][q] += K^T dS^T with dS^T out of the accumulators.
// The K tile is read both ways (pitch BP), V by rows only.
// ---------------------------------------------------------------------------------------------------------------------
template <int HD>
__global__ __launch_bounds__(256) void attn_bwd_dq_kernel(const TaArgs a) {
  using G = AttnGeom<HD>;
  __shared__ __attribute__((aligned(16))) char ks_[AT_KT * G::BP];
  __shared__ __attribute__((aligned(16))) char vs_[AT_KT * G::RP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, head = blockIdx.y;
  const int q0 = blockIdx.x * AT_QW + wave * 32;
  const size_t rowp = (size_t)3 * a.c;
  const unsigned short* base = a.qkv + (size_t)b * a.t * rowp + (size_t)head * HD;
  const int lim = key_limit<false>(a.key_len, b, a.t);
  const TileLane g = tile_lane<G::BP>(lane);
  const int query = q0 + g.n32;
  const bool q_ok = query < a.t;
  const int qrow = q_ok ? query : a.t - 1;
  const bool drop = a.p_drop > 0.f;
  const unsigned long long erow = mask_row(b, a.heads, head, a.t, qrow);
  zero_pad<HD, G::BP>(ks_, AT_KT, tid, 256);                                  // the loop's first barrier orders it before any read
  s16x8 qf[HD / 16], gf[HD / 16];
  load_row_frags(qf, base + (size_t)qrow * rowp + 8 * g.half);
  load_row_frags(gf, a.dout + ((size_t)b * a.t + qrow) * a.c + (size_t)head * HD + 8 * g.half);
  const float lse2 = a.lse2[((size_t)b * a.heads + head) * a.t + qrow], dsum = a.dsum[((size_t)b * a.heads + head) * a.t + qrow];
  f32x16 dq[(HD + 31) / 32];
#pragma unroll
  for (int mt = 0; mt < (HD + 31) / 32; ++mt) zero(dq[mt]);
  for (int k0 = 0; k0 < lim; k0 += AT_KT) {
    __syncthreads();
    stage_kv<HD, G::BP, G::RP>(ks_, vs_, base, rowp, a.c, a.t, k0, tid);
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      if (k0 + sub * 32 >= lim) break;
      f32x16 s, dp;
      qk_dp_subtile<G::BP, G::RP>(s, dp, ks_, vs_, sub, g, qf, gf);
      bwd_tile<false>(s, dp, k0 + sub * 32 + 8 * g.half, lim, q_ok, lse2, dsum, a.scale_log2e, a.keep_scale, a.mask, erow, drop);
      acc_tile_t<G::BP>(dq, dp, ks_, sub, g);
    }
  }
  if (q_ok) store_f32<HD>(a.dqkv + ((size_t)b * a.t + query) * rowp + (size_t)head * HD + 4 * g.half, dq, a.scale);
}

// ---------------------------------------------------------------------------------------------------------------------
// backward, dK and dV: the dKV sequence of csrc/attn_tile.hpp as it stands.  K and V are read by rows only (pitch RP), the wave-private Q and dO tiles
// both ways (BP).  The accumulators cover d x 64 keys twice, [d blocks][2] tiles each: 128 registers at head_dim 64, 192 at 80 -- one wave per SIMD
// either way (the register file is 512 per lane there; so is the LDS: one workgroup per CU).
// ---------------------------------------------------------------------------------------------------------------------
template <int HD>
__global__ __launch_bounds__(256) void attn_bwd_dkv_kernel(const TaArgs a) {
  using G = AttnGeom<HD>;
  constexpr int DB = (HD + 31) / 32;
  static_assert(at_dkv_lds<HD>() >= G::DKV_RED + (size_t)4 * 2 * DB * 16 * 64 * 4, "the final sums reuse the allocation from DKV_RED on");
  extern __shared__ __attribute__((aligned(16))) char sm[];
  char* const ks_ = sm;                                  // [64][RP]
  char* const vs_ = sm + AT_KT * G::RP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  char* const wt = sm + 2 * AT_KT * G::RP + wave * (2 * 32 * G::BP + 2 * AT_WTILE);  // this wave's Q, dO, Pd, dS tiles
  const int b = blockIdx.z, head = blockIdx.y, k0 = blockIdx.x * AT_KT;
  const size_t rowp = (size_t)3 * a.c;
  const unsigned short* base = a.qkv + (size_t)b * a.t * rowp + (size_t)head * HD;
  const int lim = key_limit<false>(a.key_len, b, a.t);
  const bool drop = a.p_drop > 0.f;
  const TileLane g = tile_lane(lane);
  const int tr_q = tile_lane<G::BP>(lane).tr_off;        // Q / dO tiles; g.tr_off is the Pd / dS tiles'
  stage_kv<HD, G::RP>(ks_, vs_, base, rowp, a.c, a.t, k0, tid);
  zero_pad<HD, G::BP>(wt, 32, lane, 64);                 // the wave's own stores: ordered before its reads by the loop's first wait
  zero_pad<HD, G::BP>(wt + 32 * G::BP, 32, lane, 64);
  __syncthreads();
  f32x16 dv[DB][2], dk[DB][2];                           // [d block mt][key block nt]
#pragma unroll
  for (int mt = 0; mt < DB; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int i = 0; i < 16; ++i) { dv[mt][nt][i] = 0.f; dk[mt][nt][i] = 0.f; }
  const bool any_key = k0 < lim;
  for (int q0 = wave * 32; q0 < a.t && any_key; q0 += AT_QW) {
    dkv_stage_rows<HD, G::BP>(wt, base, rowp, a.dout, b, head, a.t, a.c, q0, lane);
    const int query = q0 + g.n32;
    const bool q_ok = query < a.t;
    const int qrow = q_ok ? query : a.t - 1;
    const unsigned long long erow = mask_row(b, a.heads, head, a.t, qrow);
    const float lse2 = a.lse2[((size_t)b * a.heads + head) * a.t + qrow], dsum = a.dsum[((size_t)b * a.heads + head) * a.t + qrow];
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    s16x8 qf[HD / 16], gf[HD / 16];
    dkv_load_frags<G::BP>(qf, gf, wt, g);
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      f32x16 s, dp;
      qk_dp_subtile<G::RP>(s, dp, ks_, vs_, sub, g, qf, gf);
      bwd_tile<false>(s, dp, k0 + sub * 32 + 8 * g.half, lim, q_ok, lse2, dsum, a.scale_log2e, a.keep_scale, a.mask, erow, drop);
      dkv_store_tiles<G::BP>(wt, s, dp, sub, g);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      s16x8 ga[DB], qa[DB], pb[2], sb[2];
      dkv_operands<G::BP>(ga, qa, pb, sb, wt, ks, g, tr_q);
#pragma unroll
      for (int mt = 0; mt < DB; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
          dv[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ga[mt], pb[nt], dv[mt][nt], 0, 0, 0);
          dk[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa[mt], sb[nt], dk[mt][nt], 0, 0, 0);
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  dkv_reduce_store<HD>(reinterpret_cast<float*>(sm + G::DKV_RED), dv, dk, a.scale, a.dqkv, rowp, b, a.t, a.c, head, k0, wave, lane, g);
}

template <int HD>
TaArgs train_args(const void* qkv, int32_t t, int32_t c, int32_t heads, const int32_t* key_len, float p_drop) {
  TaArgs a{};
  a.qkv = static_cast<const unsigned short*>(qkv); a.key_len = key_len;
  a.t = t; a.c = c; a.heads = heads;
  a.scale = 1.f / sqrtf((float)HD); a.scale_log2e = LOG2E * a.scale;
  a.p_drop = p_drop; a.keep_scale = 1.f / (1.f - p_drop);
  return a;
}

template <int HD>
int train_fwd_launch(const void* qkv_bf16, int32_t batch, int32_t t, int32_t c, int32_t heads, const int32_t* key_len, float p_drop, uint64_t seed, float* ctx,
                     float* lse2, void* workspace, hipStream_t stream) {
  TaArgs a = train_args<HD>(qkv_bf16, t, c, heads, key_len, p_drop);
  a.ctx = ctx; a.lse2 = lse2;
  if (p_drop > 0.f) {
    attn_draw_mask(static_cast<unsigned*>(workspace), batch, t, heads, seed, p_drop, stream);
    a.mask = static_cast<const unsigned*>(workspace);
  }
  hipLaunchKernelGGL(attn_fwd_train_kernel<HD>, dim3((t + AT_QW - 1) / AT_QW, heads, batch), dim3(256), 0, stream, a);
  return hip_status(hipGetLastError());
}

template <int HD>
int train_bwd_launch(const void* qkv_bf16, int32_t batch, int32_t t, int32_t c, int32_t heads, const int32_t* key_len, float p_drop, uint64_t seed,
                     const float* dctx, const float* ctx, const float* lse2, const void* fwd_mask, float* dqkv, void* workspace, hipStream_t stream) {
  // the dynamic-LDS limit of the dKV kernel, once per device
  static bool attr[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return TS_EINVAL;
  if (!attr[dev]) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(attn_bwd_dkv_kernel<HD>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)at_dkv_lds<HD>()) !=
        hipSuccess)
      return TS_EUNSUPPORTED;
    attr[dev] = true;
  }
  TaArgs a = train_args<HD>(qkv_bf16, t, c, heads, key_len, p_drop);
  a.lse2 = const_cast<float*>(lse2); a.dqkv = dqkv;
  unsigned short* const dout16 = static_cast<unsigned short*>(workspace);
  float* const dsum = reinterpret_cast<float*>(static_cast<char*>(workspace) + al16((int64_t)batch * t * c * 2));
  a.dout = dout16; a.dsum = dsum;
  if (p_drop > 0.f && fwd_mask) a.mask = static_cast<const unsigned*>(fwd_mask);      // the forward's workspace, kept by the caller (4 MB per layer at 8 x 10 s)
  else if (p_drop > 0.f) {                                                            // or re-drawn: the mask is a pure function of the seed
    unsigned* const mask = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(dsum) + al16((int64_t)batch * heads * t * 4));
    attn_draw_mask(mask, batch, t, heads, seed, p_drop, stream);
    a.mask = mask;
  }
  if constexpr (HD == 64) attn_rowdot(dctx, ctx, dout16, dsum, batch, t, c, heads, stream);
  else {
    const long long units = (long long)batch * t * heads;
    hipLaunchKernelGGL(attn_rowdot80_kernel, dim3((unsigned)((units + 63) / 64)), dim3(256), 0, stream, dctx, ctx, dout16, dsum, units, t, c, heads);
  }
  hipLaunchKernelGGL(attn_bwd_dq_kernel<HD>, dim3((t + AT_QW - 1) / AT_QW, heads, batch), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(attn_bwd_dkv_kernel<HD>, dim3((t + AT_KT - 1) / AT_KT, heads, batch), dim3(256), at_dkv_lds<HD>(), stream, a);
  return hip_status(hipGetLastError());
}

}  // namespace

int attn_train_check(const void* qkv, int32_t batch, int32_t t, int32_t c, int32_t heads, float p_drop) {
  if (!qkv || batch <= 0 || t <= 0 || c <= 0 || heads <= 0 || c % heads || !(p_drop >= 0.f && p_drop < 1.f)) return TS_EINVAL;
  if (c / heads != 64 || c % 8 || misaligned(qkv) || (long long)batch * heads * t * t >= (1ll << 40)) return TS_EUNSUPPORTED;
  return TS_OK;
}

// words of the mask bitstring: every element + four words of slack.  The dKV kernels run bwd_tile over whole 64-key tiles, keys past t included,
// so with N = batch heads t t elements the furthest read belongs to the last row (first element N - t) in the last key tile (k0 <= t - 1) at sub = 1,
// half = 1, second run of 8: e0 = N - t + k0 + 32 + 8 + 16 <= N + 55, and keep8 reads words e0 / 32 and e0 / 32 + 1 <= ceil(N / 32) + 2 -- the
// third word past the last one that holds an element (those bits land on masked keys); the fourth is spare.
long long attn_mask_words(int batch, int t, int heads) { return ((long long)batch * heads * t * t + 31) / 32 + 4; }

void attn_draw_mask(unsigned* mask, int batch, int t, int heads, unsigned long long seed, float p, hipStream_t stream) {
  const long long n = attn_mask_words(batch, t, heads);
  hipLaunchKernelGGL(attn_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, mask, n, seed, p);
}

void attn_rowdot(const float* dctx, const float* ctx, unsigned short* dout16, float* dsum, int batch, int t, int c, int heads, hipStream_t stream) {
  const long long rows = (long long)batch * t;
  hipLaunchKernelGGL(attn_rowdot_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, dctx, ctx, dout16, dsum, rows, t, c, heads);
}

int64_t attn_train_fwd_workspace(int32_t batch, int32_t t, int32_t c, int32_t heads) {
  if (batch <= 0 || t <= 0 || c <= 0 || heads <= 0) return TS_EINVAL;
  return al16(attn_mask_words(batch, t, heads) * 4);
}

int64_t attn_train_bwd_workspace(int32_t batch, int32_t t, int32_t c, int32_t heads) {
  if (batch <= 0 || t <= 0 || c <= 0 || heads <= 0) return TS_EINVAL;
  return al16((int64_t)batch * t * c * 2) + al16((int64_t)batch * heads * t * 4) + al16(attn_mask_words(batch, t, heads) * 4);
}

int attn_train_fwd_launch(int hd, const void* qkv_bf16, int32_t batch, int32_t t, int32_t c, int32_t heads, const int32_t* key_len, float p_drop, uint64_t seed,
                          float* ctx, float* lse2, void* workspace, hipStream_t stream) {
  return hd == 64 ? train_fwd_launch<64>(qkv_bf16, batch, t, c, heads, key_len, p_drop, seed, ctx, lse2, workspace, stream)
                  : train_fwd_launch<80>(qkv_bf16, batch, t, c, heads, key_len, p_drop, seed, ctx, lse2, workspace, stream);
}

int attn_train_bwd_launch(int hd, const void* qkv_bf16, int32_t batch, int32_t t, int32_t c, int32_t heads, const int32_t* key_len, float p_drop, uint64_t seed,
                          const float* dctx, const float* ctx, const float* lse2, const void* fwd_mask, float* dqkv, void* workspace, hipStream_t stream) {
  return hd == 64 ? train_bwd_launch<64>(qkv_bf16, batch, t, c, heads, key_len, p_drop, seed, dctx, ctx, lse2, fwd_mask, dqkv, workspace, stream)
                  : train_bwd_launch<80>(qkv_bf16, batch, t, c, heads, key_len, p_drop, seed, dctx, ctx, lse2, fwd_mask, dqkv, workspace, stream);
}

}  // namespace ts

using namespace ts;

/* see include/thunder_speech_amd.h */
extern "C" int64_t ts_w2v_attention_train_fwd_workspace(int32_t batch, int32_t t, int32_t c, int32_t heads) {
  return attn_train_fwd_workspace(batch, t, c, heads);
}

extern "C" int ts_w2v_attention_train_fwd(const void* qkv_bf16, int32_t batch, int32_t t, int32_t c, int32_t heads, const int32_t* key_len, float p_drop,
                                          uint64_t seed, float* ctx, float* lse2, void* workspace, void* stream_) {
  if (int st = attn_train_check(qkv_bf16, batch, t, c, heads, p_drop)) return st;
  if (!ctx || !lse2 || misaligned(ctx) || (p_drop > 0.f && (!workspace || misaligned(workspace)))) return TS_EINVAL;
  TS_STREAM;
  return attn_train_fwd_launch(64, qkv_bf16, batch, t, c, heads, key_len, p_drop, seed, ctx, lse2, workspace, stream);
}

extern "C" int64_t ts_w2v_attention_train_bwd_workspace(int32_t batch, int32_t t, int32_t c, int32_t heads) {
  return attn_train_bwd_workspace(batch, t, c, heads);
}

/* see include/thunder_speech_amd.h */
extern "C" int ts_w2v_attention_train_bwd(const void* qkv_bf16, int32_t batch, int32_t t, int32_t c, int32_t heads, const int32_t* key_len, float p_drop,
                                          uint64_t seed, const float* dctx, const float* ctx, const float* lse2, const void* fwd_mask, float* dqkv, void* workspace,
                                          void* stream_) {
  if (int st = attn_train_check(qkv_bf16, batch, t, c, heads, p_drop)) return st;
  if (!dctx || !ctx || !lse2 || !dqkv || !workspace) return TS_EINVAL;
  if (misaligned(dctx) || misaligned(ctx) || misaligned(dqkv) || misaligned(workspace)) return TS_EUNSUPPORTED;
  TS_STREAM;
  return attn_train_bwd_launch(64, qkv_bf16, batch, t, c, heads, key_len, p_drop, seed, dctx, ctx, lse2, fwd_mask, dqkv, workspace, stream);
}
