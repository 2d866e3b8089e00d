// Fused self-attention for mixed-precision FINE-TUNING at head_dim 80 (XLS-R 1B / MMS: hidden 1280, 16 heads): forward and backward without the
// [T][T] score / probability matrices of the unfused path (huggingface/train.py Attention).  include/thunder_speech_amd_mms_train.h is the ABI; the
// contract is ts_w2v_attention_train_fwd / _bwd's (csrc/w2v_attn_train.hip) with scale = 1 / sqrt(80):
//   forward   (mt_fwd_kernel)      mms_flash_attn_kernel's sequence (csrc/mms.hip) + the dropout keep bits of ts_train_dropout (element
//             e = ((b H + h) T + q) T + k, bit e of the bitstring attn_mask_kernel draws) + f32 ctx + the row statistic lse2 = max + log2(sum);
//   backward  mt_rowdot_kernel     D[b][h][q] = sum_d dO O over the head's 80 columns, and the bf16 copy of dO;
//             mt_bwd_dq_kernel     workgroup = 128 queries, loop over key tiles:   dQ^T[d][q] += K^T dS^T;
//             mt_bwd_dkv_kernel    workgroup = 64 keys, loop over query tiles:     dV += Pd^T dO,  dK += dS^T Q  (P / dS through wave-private LDS);
//             with dP = (dO V^T) * keep / (1 - p),  dS = P * (dP - D).  Both rebuild the probabilities as exp2(s c - lse2): no atomics, fixed order.
// Operands bf16 (q, k, v, dO, P, dS), softmax arithmetic and accumulation f32, results f32 (ctx, dqkv).
//
// From csrc/attn_tile.hpp come the pieces that do not know the head dimension (key_limit, tile_lane, mask_tail, softmax_step, zero, keep8 / drop_keys,
// bwd_tile) and the host side of the mask (attn_mask_words, attn_draw_mask: the tiles are 64 keys x 32-key sub-tiles as there, so the mask's slack words
// cover these kernels' reads too).  The tile helpers below are this file's own, templated on the LDS pitch of the tile they read.
//
// Geometry: a first product (S^T = K Q^T, dP^T = V dO^T) takes five k-steps (80 = 5 x 16) and reads its tile by rows (ds_read_b128); a second product
// (O^T += V^T P^T, dQ^T += K^T dS^T, dV^T += dO^T Pd, dK^T += Q^T dS) covers d in three 32-row blocks, 0..95, and reads its tile transposed
// (ds_read_b64_tr_b16).  Rows 80..95 of the third block belong to no output: an MFMA A row feeds only its own output row, so those columns of a tile only
// have to be legal to read.  Every tile that is read transposed is 96 columns wide or wider, its pad columns 80..95 are zeroed once, and every epilogue
// stores d < 80 only (head h's columns end where head h + 1's begin).
//
// LDS pitches, by the bank rules of mms.hip (bank = dword address mod 64; a b128 read is served per 16-lane group, which reads rows of all 16 residues
// mod 16 at one column; a transposing b64 read per 32-lane half, which reads 4 rows x 16 consecutive dwords, and once more 4 rows further down):
//   rows only (forward K; dQ kernel V; dKV kernel K and V):  176 bytes = 44 dwords, conflict-free (4 x odd).
//   transposed only (forward V):  192 bytes = 48 dwords, conflict-free (the four rows start at banks 0, 48, 32, 16).
//   BOTH (dQ kernel K; dKV kernel's wave-private Q and dO tiles):  no pitch serves both.  The b128 rule needs pitch = 4 x odd dwords, i.e. pitch mod 16
//     in {4, 12}.  The transposing read needs the 16-bank windows that start at 0, P, 2P, 3P (mod 64) disjoint; four windows of 16 on a ring of 64 are
//     disjoint only when they tile it, P mod 64 in {16, 48} -- a multiple of 16, never 4 x odd.  These tiles take 208 bytes = 52 dwords (the smallest
//     4 x odd pitch that holds 96 columns): the b128 row reads are conflict-free, and the TRANSPOSING read pays: its windows start at banks 0, 52, 40, 28,
//     so neighbouring rows overlap on 4 banks each (0-3, 52-55, 40-43): 12 of the 64 banks are hit two ways, the other 52 once.  The other choice, 192
//     bytes, would make every b128 read four ways (48 r mod 64 takes 4 values over 16 rows); a sub-tile issues 10 b128 and 12 transposing reads.
//   dKV kernel's Pd / dS tiles (written as b128 rows, read transposed, 64 columns):  AT_PITCH = 144 bytes, as the head_dim 64 kernel.
#include "attn_tile.hpp"
#include "thunder_speech_amd_mms_train.h"

namespace ts {

namespace {

constexpr int MT_HD = 80;
constexpr int MT_RP = 176;                       // bytes per row of a tile read by rows only
constexpr int MT_TP = 192;                       // ... read transposed only: 96 bf16
constexpr int MT_BP = 208;                       // ... read both ways
constexpr int MT_CHUNKS = AT_KT * (MT_HD / 8);   // 16-byte chunks of one staged 64-row tile: 640 for 256 threads
// dKV kernel: K, V (rows only) + per wave Q | dO (32 rows, both ways) | Pd | dS (32 rows, AT_PITCH)
constexpr int MT_WQ = 32 * MT_BP;
constexpr int MT_WAVE = 2 * MT_WQ + 2 * AT_WTILE;
constexpr size_t MT_DKV_LDS = (size_t)2 * AT_KT * MT_RP + (size_t)4 * MT_WAVE;          // 110 KiB; one round of the final sums needs 96 of them
static_assert(MT_DKV_LDS >= (size_t)4 * 6 * 16 * 64 * 4, "the final sums of mt_bwd_dkv_kernel reuse the whole allocation");

struct MtArgs {
  const unsigned short* qkv;       // [B][T][3C] bf16
  const int* key_len;
  float* ctx;                      // forward: [B][T][C] f32
  float* lse2;                     // [B][H][T]
  const unsigned short* dout;      // backward: [B][T][C] bf16
  const float* dsum;               // backward: D [B][H][T]
  float* dqkv;                     // backward: [B][T][3C] f32
  int t, c, heads;
  float scale_log2e, scale;        // log2(e) / sqrt(80), 1 / sqrt(80)
  float p_drop, keep_scale;        // dropout probability, 1 / (1 - p)
  const unsigned* mask;            // keep bits of the whole [B H T][T] dropout stream (attn_mask_kernel); NULL when p_drop == 0
};

// K and V rows k0 .. k0 + 63 of one (clip, head) into LDS, 10 chunks of 16 bytes per row (rows past t clamped to t - 1: their probabilities are 0)
template <int KP, int VP>
__device__ __forceinline__ void mt_stage_kv(char* ks_, char* vs_, const unsigned short* base, size_t rowp, int c, int t, int k0, int tid) {
#pragma unroll
  for (int rep = 0; rep < 3; ++rep) {
    const int chunk = tid + 256 * rep;
    if (chunk < MT_CHUNKS) {
      const int r = chunk / 10, cc = chunk - 10 * r;
      const int key = k0 + r < t ? k0 + r : t - 1;
      const unsigned short* src = base + (size_t)key * rowp + cc * 8;
      *reinterpret_cast<uint4*>(ks_ + r * KP + cc * 16) = *reinterpret_cast<const uint4*>(src + c);
      *reinterpret_cast<uint4*>(vs_ + r * VP + cc * 16) = *reinterpret_cast<const uint4*>(src + 2 * c);
    }
  }
}

// the pad columns 80 .. 95 of `rows` tile rows (two 16-byte chunks per row), by the first 2 rows of `n` threads
template <int P>
__device__ __forceinline__ void mt_zero_pad(char* tile, int rows, int idx, int n) {
  for (int i = idx; i < 2 * rows; i += n) *reinterpret_cast<uint4*>(tile + (i >> 1) * P + (10 + (i & 1)) * 16) = uint4{0u, 0u, 0u, 0u};
}

// B operand of the first products, lane = (query n32, k-half): 8 consecutive d per k-step, from the row's 80 bf16 at p = row + 8 half
__device__ __forceinline__ void mt_load_row_frags(s16x8 (&f)[5], const unsigned short* p) {
  const uint4* p4 = reinterpret_cast<const uint4*>(p);
#pragma unroll
  for (int ks = 0; ks < 5; ++ks) f[ks] = __builtin_bit_cast(s16x8, p4[2 * ks]);
}

// acc^T[row of the tile][query] = tile x^T over d, five k-steps, for the 32 rows of sub-tile `sub`; accumulator register
// i <-> row 32 sub + 16 (i / 8) + 8 half + i % 8 (the order mask_tail / bwd_tile expect)
template <int P>
__device__ __forceinline__ f32x16 mt_rows_product(const char* tile, int sub, const TileLane& g, const s16x8 (&xf)[5]) {
  f32x16 s;
  zero(s);
  const char* r = tile + (sub * 32 + g.pm) * P + g.half * 16;
#pragma unroll
  for (int ks = 0; ks < 5; ++ks) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const s16x8*>(r + ks * 32), xf[ks], s, 0, 0, 0);
  return s;
}

// tile_lane's tr_off at pitch P
template <int P>
__device__ __forceinline__ int mt_tr_off(int lane) {
  return (8 * (lane >> 5) + ((lane >> 2) & 3)) * P + (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;
}

// two ds_read_b64_tr_b16: the 8 operand elements of one k-step of 16 rows, transposed out of a row-major tile of pitch P
template <int P>
__device__ __forceinline__ s16x8 mt_tr8(const char* p) {
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((TS_LDS s16x4*)((TS_LDS char*)p));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((TS_LDS s16x4*)((TS_LDS char*)p + 4 * P));
  return s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

__device__ __forceinline__ s16x8 mt_pack8(const f32x16& x, int run) {
  return __builtin_bit_cast(s16x8, uint4{pack_bf16(x[8 * run + 0], x[8 * run + 1]), pack_bf16(x[8 * run + 2], x[8 * run + 3]),
                                         pack_bf16(x[8 * run + 4], x[8 * run + 5]), pack_bf16(x[8 * run + 6], x[8 * run + 7])});
}

// acc^T[d][query] += tile^T x^T over the 32 keys of sub-tile `sub`: x (P, or dS) goes from the accumulators to the bf16 B operand, the staged [key][d]
// tile (V, or K) is read transposed; acc[mt] holds d = 32 mt .. 32 mt + 31 (d >= 80: the zeroed pad columns)
template <int P>
__device__ __forceinline__ void mt_acc_t(f32x16 (&acc)[3], const f32x16& x, const char* tile, int sub, int tr_off) {
#pragma unroll
  for (int ks2 = 0; ks2 < 2; ++ks2) {
    const s16x8 xb = mt_pack8(x, ks2);
#pragma unroll
    for (int mt = 0; mt < 3; ++mt)
      acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(mt_tr8<P>(tile + (sub * 32 + 16 * ks2) * P + tr_off + 64 * mt), xb, acc[mt], 0, 0, 0);
  }
}

// epilogue of the forward / dQ kernels, dst = the lane's output row + 80 head + 4 half: accumulator registers 4 gg .. 4 gg + 3 of block mt <-> d =
// 32 mt + 8 gg + 4 half + 0..3; the third block stops at d = 80
__device__ __forceinline__ void mt_store_f32(float* dst, const f32x16 (&o)[3], float mul) {
#pragma unroll
  for (int mt = 0; mt < 3; ++mt)
#pragma unroll
    for (int gg = 0; gg < (mt < 2 ? 4 : 2); ++gg)
      *reinterpret_cast<f32x4*>(dst + 32 * mt + 8 * gg) = f32x4{o[mt][4 * gg] * mul, o[mt][4 * gg + 1] * mul, o[mt][4 * gg + 2] * mul, o[mt][4 * gg + 3] * mul};
}

__device__ __forceinline__ unsigned long long mt_erow(int b, int heads, int head, int t, int qrow) {
  return (((unsigned long long)b * heads + head) * t + qrow) * (unsigned long long)t;
}

// ---------------------------------------------------------------------------------------------------------------------
// forward.  amdgpu_waves_per_eu(3, 3): the loop is bound by the softmax's quarter-rate exp2, which only other resident waves hide, but the budget
// of 4 waves that mms_flash_attn_kernel takes leaves this kernel (which also carries the dropout row index and the mask pointer) 7 spilled VGPRs with
// one reload inside the key loop; at 3 the compiler reports 151 VGPRs and no scratch.  All four kernels' reports: profiles/xlsr1b_finetune.md.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void mt_fwd_kernel(const MtArgs a) {
  __shared__ __attribute__((aligned(16))) char ks_[AT_KT * MT_RP];
  __shared__ __attribute__((aligned(16))) char vs_[AT_KT * MT_TP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, head = blockIdx.y;
  const int q0 = blockIdx.x * AT_QW + wave * 32;
  const size_t rowp = (size_t)3 * a.c;
  const unsigned short* base = a.qkv + (size_t)b * a.t * rowp + (size_t)head * MT_HD;
  const int lim = key_limit<false>(a.key_len, b, a.t);
  const TileLane g = tile_lane(lane);
  const int tr_off = mt_tr_off<MT_TP>(lane);
  const int query = q0 + g.n32;
  const int qrow = query < a.t ? query : a.t - 1;
  const bool drop = a.p_drop > 0.f;
  const unsigned long long erow = mt_erow(b, a.heads, head, a.t, qrow);
  mt_zero_pad<MT_TP>(vs_, AT_KT, tid, 256);                                   // the loop's first barrier orders it before any read
  s16x8 qf[5];
  mt_load_row_frags(qf, base + (size_t)qrow * rowp + 8 * g.half);
  f32x16 o[3];
  zero(o[0]); zero(o[1]); zero(o[2]);
  float m_run = -INFINITY, l_run = 0.f;

  for (int k0 = 0; k0 < lim; k0 += AT_KT) {
    __syncthreads();                                                          // the previous tile has been consumed
    mt_stage_kv<MT_RP, MT_TP>(ks_, vs_, base, rowp, a.c, a.t, k0, tid);
    __syncthreads();
    const bool full = k0 + AT_KT <= lim;                                      // no masked key in this tile (uniform)
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      if (k0 + sub * 32 >= lim) break;                                        // uniform: nothing but masked keys
      f32x16 s = mt_rows_product<MT_RP>(ks_, sub, g, qf);
      const int kbase = k0 + sub * 32 + 8 * g.half;
      if (!full) s = mask_tail(s, kbase, lim);
      const SoftmaxStep sm = softmax_step<true>(s, m_run, l_run, a.scale_log2e);
      m_run = sm.m; l_run = sm.l;
      const f32x16 p = drop ? drop_keys(sm.p, a.mask, erow + kbase, a.keep_scale) : sm.p;
      if (__any(sm.alpha != 1.f)) {                                           // after the first tiles the running maximum rarely moves
#pragma unroll
        for (int mt = 0; mt < 3; ++mt)
#pragma unroll
          for (int i = 0; i < 16; ++i) o[mt][i] *= sm.alpha;
      }
      mt_acc_t<MT_TP>(o, p, vs_, sub, tr_off);
    }
  }
  const float l = l_run + __shfl_xor(l_run, 32);
  const float inv = l > 0.f ? 1.f / l : 0.f;     // (no valid key: zeros, and a row statistic that makes every rebuilt probability 0)
  if (query < a.t) {
    mt_store_f32(a.ctx + ((size_t)b * a.t + query) * a.c + (size_t)head * MT_HD + 4 * g.half, o, inv);
    if (g.half == 0) a.lse2[((size_t)b * a.heads + head) * a.t + query] = l > 0.f ? m_run + __builtin_amdgcn_logf(l) : INFINITY;      // v_log_f32 = log2
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// backward, part 0: bf16 copy of dO and D[b][h][q] = sum_d dO[q][d] O[q][d] over the head's 80 columns.  Four lanes per (b, q, head): lane j of
// the four takes columns 16 i + 4 j .. + 3 for i = 0 .. 4 (a quad reads 64 consecutive bytes per step), then two exchanges inside the quad.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mt_rowdot_kernel(const float* __restrict__ dout, const float* __restrict__ ctx, unsigned short* __restrict__ dout16,
                                                        float* __restrict__ dsum, long long units, int t, int c, int heads) {
  const long long unit = (long long)blockIdx.x * 64 + (threadIdx.x >> 2);      // (b t + q) heads + h
  if (unit >= units) return;                                                   // whole quads leave together
  const int j = threadIdx.x & 3;
  const long long row = unit / heads;
  const int h = (int)(unit - row * heads);
  const long long b = row / t;
  const int q = (int)(row - b * t);
  const size_t off = (size_t)row * c + (size_t)h * MT_HD + 4 * j;
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
// The K tile is read both ways (pitch MT_BP), V by rows only.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mt_bwd_dq_kernel(const MtArgs a) {
  __shared__ __attribute__((aligned(16))) char ks_[AT_KT * MT_BP];
  __shared__ __attribute__((aligned(16))) char vs_[AT_KT * MT_RP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, head = blockIdx.y;
  const int q0 = blockIdx.x * AT_QW + wave * 32;
  const size_t rowp = (size_t)3 * a.c;
  const unsigned short* base = a.qkv + (size_t)b * a.t * rowp + (size_t)head * MT_HD;
  const int lim = key_limit<false>(a.key_len, b, a.t);
  const TileLane g = tile_lane(lane);
  const int tr_off = mt_tr_off<MT_BP>(lane);
  const int query = q0 + g.n32;
  const bool q_ok = query < a.t;
  const int qrow = q_ok ? query : a.t - 1;
  const bool drop = a.p_drop > 0.f;
  const unsigned long long erow = mt_erow(b, a.heads, head, a.t, qrow);
  mt_zero_pad<MT_BP>(ks_, AT_KT, tid, 256);                                   // the loop's first barrier orders it before any read
  s16x8 qf[5], gf[5];
  mt_load_row_frags(qf, base + (size_t)qrow * rowp + 8 * g.half);
  mt_load_row_frags(gf, a.dout + ((size_t)b * a.t + qrow) * a.c + (size_t)head * MT_HD + 8 * g.half);
  const float lse2 = a.lse2[((size_t)b * a.heads + head) * a.t + qrow], dsum = a.dsum[((size_t)b * a.heads + head) * a.t + qrow];
  f32x16 dq[3];
  zero(dq[0]); zero(dq[1]); zero(dq[2]);
  for (int k0 = 0; k0 < lim; k0 += AT_KT) {
    __syncthreads();
    mt_stage_kv<MT_BP, MT_RP>(ks_, vs_, base, rowp, a.c, a.t, k0, tid);
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      if (k0 + sub * 32 >= lim) break;
      f32x16 s = mt_rows_product<MT_BP>(ks_, sub, g, qf);
      f32x16 dp = mt_rows_product<MT_RP>(vs_, sub, g, gf);
      bwd_tile<false>(s, dp, k0 + sub * 32 + 8 * g.half, lim, q_ok, lse2, dsum, a.scale_log2e, a.keep_scale, a.mask, erow, drop);
      mt_acc_t<MT_BP>(dq, dp, ks_, sub, tr_off);
    }
  }
  if (q_ok) mt_store_f32(a.dqkv + ((size_t)b * a.t + query) * rowp + (size_t)head * MT_HD + 4 * g.half, dq, a.scale);
}

// ---------------------------------------------------------------------------------------------------------------------
// backward, dK and dV: workgroup = 64 keys of one (clip, head), loop over 128-query tiles (32 per wave).  Per wave and tile the Q and dO rows are
// staged in wave-private LDS (wt: Q | dO at pitch MT_BP, Pd | dS at AT_PITCH), P * keep / (1 - p) and dS go there as bf16 [query][key] tiles, and
//   dV^T[d][key] += dO^T[d][q] Pd[q][key],   dK^T[d][key] += Q^T[d][q] dS[q][key]
// take both operands out of those tiles with transposing reads (contraction over the tile's 32 queries).  The accumulators cover d 0..95 x 64 keys
// twice: [3][2] tiles each, 192 registers -- one wave per SIMD (the register file is 512 per lane there; so is the LDS: one workgroup per CU).
// The tiles are wave-private and LDS operations of a wave execute in order: an s_waitcnt + wave_barrier pair between the phases is all the loop needs.
// The four waves' sums meet in LDS at the end, in a fixed order.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mt_bwd_dkv_kernel(const MtArgs a) {
  extern __shared__ __attribute__((aligned(16))) char sm[];
  char* const ks_ = sm;                                    // [64][MT_RP]
  char* const vs_ = sm + AT_KT * MT_RP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  char* const wq = sm + 2 * AT_KT * MT_RP + wave * MT_WAVE;  // this wave's Q, dO, Pd, dS tiles
  char* const wg = wq + MT_WQ;
  char* const wp = wq + 2 * MT_WQ;
  char* const wd = wp + AT_WTILE;
  const int b = blockIdx.z, head = blockIdx.y, k0 = blockIdx.x * AT_KT;
  const size_t rowp = (size_t)3 * a.c;
  const unsigned short* base = a.qkv + (size_t)b * a.t * rowp + (size_t)head * MT_HD;
  const int lim = key_limit<false>(a.key_len, b, a.t);
  const bool drop = a.p_drop > 0.f;
  const TileLane g = tile_lane(lane);
  const int tr_q = mt_tr_off<MT_BP>(lane);                 // Q / dO tiles; g.tr_off is the Pd / dS tiles'
  mt_stage_kv<MT_RP, MT_RP>(ks_, vs_, base, rowp, a.c, a.t, k0, tid);
  mt_zero_pad<MT_BP>(wq, 32, lane, 64);                    // the wave's own stores: ordered before its reads by the loop's first wait
  mt_zero_pad<MT_BP>(wg, 32, lane, 64);
  __syncthreads();
  f32x16 dv[3][2], dk[3][2];                               // [d block mt][key block nt]
#pragma unroll
  for (int mt = 0; mt < 3; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int i = 0; i < 16; ++i) { dv[mt][nt][i] = 0.f; dk[mt][nt][i] = 0.f; }
  const bool any_key = k0 < lim;
  for (int q0 = wave * 32; q0 < a.t && any_key; q0 += AT_QW) {
    // the wave's 32 Q and dO rows, 10 chunks of 16 bytes each (rows past t clamped to t - 1: q_ok zeroes their probabilities)
#pragma unroll
    for (int rep = 0; rep < 5; ++rep) {
      const int chunk = lane + 64 * rep, r = chunk / 10, cc = chunk - 10 * r;
      const int qr = q0 + r < a.t ? q0 + r : a.t - 1;
      *reinterpret_cast<uint4*>(wq + r * MT_BP + cc * 16) = *reinterpret_cast<const uint4*>(base + (size_t)qr * rowp + cc * 8);
      *reinterpret_cast<uint4*>(wg + r * MT_BP + cc * 16) =
          *reinterpret_cast<const uint4*>(a.dout + ((size_t)b * a.t + qr) * a.c + (size_t)head * MT_HD + cc * 8);
    }
    const int query = q0 + g.n32;
    const bool q_ok = query < a.t;
    const int qrow = q_ok ? query : a.t - 1;
    const unsigned long long erow = mt_erow(b, a.heads, head, a.t, qrow);
    const float lse2 = a.lse2[((size_t)b * a.heads + head) * a.t + qrow], dsum = a.dsum[((size_t)b * a.heads + head) * a.t + qrow];
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    s16x8 qf[5], gf[5];
#pragma unroll
    for (int ks = 0; ks < 5; ++ks) {
      qf[ks] = *reinterpret_cast<const s16x8*>(wq + g.n32 * MT_BP + (16 * ks + 8 * g.half) * 2);
      gf[ks] = *reinterpret_cast<const s16x8*>(wg + g.n32 * MT_BP + (16 * ks + 8 * g.half) * 2);
    }
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      f32x16 s = mt_rows_product<MT_RP>(ks_, sub, g, qf);
      f32x16 dp = mt_rows_product<MT_RP>(vs_, sub, g, gf);
      bwd_tile<false>(s, dp, k0 + sub * 32 + 8 * g.half, lim, q_ok, lse2, dsum, a.scale_log2e, a.keep_scale, a.mask, erow, drop);
      // Pd (s) and dS (dp) into the wave's tiles: row = this lane's query, columns = the keys of its two runs of 8: 32 sub + 8 half + 0..7 and + 16
#pragma unroll
      for (int run = 0; run < 2; ++run) {
        const int col = (32 * sub + 16 * run + 8 * g.half) * 2;
        *reinterpret_cast<s16x8*>(wp + g.n32 * AT_PITCH + col) = mt_pack8(s, run);
        *reinterpret_cast<s16x8*>(wd + g.n32 * AT_PITCH + col) = mt_pack8(dp, run);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {                       // contraction over the tile's 32 queries, two k-steps of 16
      s16x8 ga[3], qa[3], pb[2], sb[2];
#pragma unroll
      for (int x = 0; x < 3; ++x) {
        ga[x] = mt_tr8<MT_BP>(wg + 16 * ks * MT_BP + tr_q + 64 * x);
        qa[x] = mt_tr8<MT_BP>(wq + 16 * ks * MT_BP + tr_q + 64 * x);
      }
#pragma unroll
      for (int x = 0; x < 2; ++x) {
        pb[x] = mt_tr8<AT_PITCH>(wp + 16 * ks * AT_PITCH + g.tr_off + 64 * x);
        sb[x] = mt_tr8<AT_PITCH>(wd + 16 * ks * AT_PITCH + g.tr_off + 64 * x);
      }
#pragma unroll
      for (int mt = 0; mt < 3; ++mt)
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
  // the four waves' sums: red = [wave][block = 2 mt + nt][16][64 lanes] f32 over the whole (now idle) allocation, 96 KiB a round: dv, then dk scaled.
  // Wave w finishes blocks w and w + 4 and writes them to dqkv's V (K) third.
  float* const red = reinterpret_cast<float*>(sm);
#pragma unroll
  for (int which = 0; which < 2; ++which) {
#pragma unroll
    for (int mt = 0; mt < 3; ++mt)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int i = 0; i < 16; ++i) red[(((size_t)wave * 6 + mt * 2 + nt) * 16 + i) * 64 + lane] = which ? dk[mt][nt][i] : dv[mt][nt][i];
    __syncthreads();
    for (int blk = wave; blk < 6; blk += 4) {
      const int mt = blk >> 1, nt = blk & 1;
      f32x16 tot;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        // waves 0, 1, 2, 3 in this order, pinned: -ffast-math lets the compiler reassociate the sum, it chooses by context, and the bits of
        // dK and dV depend on the choice
#pragma clang fp reassociate(off)
        const float* part = red + ((size_t)blk * 16 + i) * 64 + lane;            // wave w's partial sum: part[w * 6144]
        const float v = ((part[0] + part[1 * 6144]) + part[2 * 6144]) + part[3 * 6144];
        tot[i] = which ? v * a.scale : v;
      }
      // accumulator register r of block (mt, nt): d = 32 mt + (r & 3) + 8 (r >> 2) + 4 half, key = k0 + 32 nt + n32; the third d block stops at 80
      const int key = k0 + 32 * nt + g.n32;
      if (key < a.t) {
        float* dst = a.dqkv + ((size_t)b * a.t + key) * rowp + (size_t)(which ? 1 : 2) * a.c + (size_t)head * MT_HD + 32 * mt + 4 * g.half;
#pragma unroll
        for (int gg = 0; gg < 4; ++gg)
          if (mt < 2 || gg < 2) *reinterpret_cast<f32x4*>(dst + 8 * gg) = f32x4{tot[4 * gg], tot[4 * gg + 1], tot[4 * gg + 2], tot[4 * gg + 3]};
      }
    }
    __syncthreads();
  }
}

int mt_check(const void* qkv, int32_t batch, int32_t t, int32_t c, int32_t heads, float p_drop) {
  if (!qkv || batch <= 0 || t <= 0 || c <= 0 || heads <= 0 || c % heads || !(p_drop >= 0.f && p_drop < 1.f)) return TS_EINVAL;
  if (c / heads != MT_HD || misaligned(qkv) || heads > 65535 || batch > 65535 || (long long)batch * heads * t * t >= (1ll << 40)) return TS_EUNSUPPORTED;
  return TS_OK;
}

MtArgs mt_args(const void* qkv, int32_t t, int32_t c, int32_t heads, const int32_t* key_len, float p_drop) {
  MtArgs a{};
  a.qkv = static_cast<const unsigned short*>(qkv); a.key_len = key_len;
  a.t = t; a.c = c; a.heads = heads;
  a.scale = 1.f / sqrtf((float)MT_HD); a.scale_log2e = LOG2E * a.scale;
  a.p_drop = p_drop; a.keep_scale = 1.f / (1.f - p_drop);
  return a;
}

}  // namespace

}  // namespace ts

using namespace ts;

extern "C" int ts_mms_train_abi_version(void) { return TS_MMS_TRAIN_ABI_VERSION; }

/* see include/thunder_speech_amd_mms_train.h */
extern "C" int64_t ts_mms_attention_train_fwd_workspace(int32_t batch, int32_t t, int32_t c, int32_t heads) {
  if (batch <= 0 || t <= 0 || c <= 0 || heads <= 0) return TS_EINVAL;
  return al16(attn_mask_words(batch, t, heads) * 4);
}

extern "C" int ts_mms_attention_train_fwd(const void* qkv_bf16, int32_t batch, int32_t t, int32_t c, int32_t heads, const int32_t* key_len, float p_drop,
                                          uint64_t seed, float* ctx, float* lse2, void* workspace, void* stream_) {
  if (int st = mt_check(qkv_bf16, batch, t, c, heads, p_drop)) return st;
  if (!ctx || !lse2 || (p_drop > 0.f && !workspace)) return TS_EINVAL;
  if (misaligned(ctx) || misaligned(lse2, 3) || misaligned(workspace) || misaligned(key_len, 3)) return TS_EUNSUPPORTED;
  TS_STREAM;
  MtArgs a = mt_args(qkv_bf16, t, c, heads, key_len, p_drop);
  a.ctx = ctx; a.lse2 = lse2;
  if (p_drop > 0.f) {
    attn_draw_mask(static_cast<unsigned*>(workspace), batch, t, heads, seed, p_drop, stream);
    a.mask = static_cast<const unsigned*>(workspace);
  }
  hipLaunchKernelGGL(mt_fwd_kernel, dim3((t + AT_QW - 1) / AT_QW, heads, batch), dim3(256), 0, stream, a);
  return hip_status(hipGetLastError());
}

// workspace: dO bf16 [B][t][c] | D f32 [B][H][t] | the mask bits (used when fwd_mask is NULL and p_drop > 0)
extern "C" int64_t ts_mms_attention_train_bwd_workspace(int32_t batch, int32_t t, int32_t c, int32_t heads) {
  if (batch <= 0 || t <= 0 || c <= 0 || heads <= 0) return TS_EINVAL;
  return al16((int64_t)batch * t * c * 2) + al16((int64_t)batch * heads * t * 4) + al16(attn_mask_words(batch, t, heads) * 4);
}

extern "C" int ts_mms_attention_train_bwd(const void* qkv_bf16, int32_t batch, int32_t t, int32_t c, int32_t heads, const int32_t* key_len, float p_drop,
                                          uint64_t seed, const float* dctx, const float* ctx, const float* lse2, const void* fwd_mask, float* dqkv,
                                          void* workspace, void* stream_) {
  if (int st = mt_check(qkv_bf16, batch, t, c, heads, p_drop)) return st;
  if (!dctx || !ctx || !lse2 || !dqkv || !workspace) return TS_EINVAL;
  if (misaligned(dctx) || misaligned(ctx) || misaligned(lse2, 3) || misaligned(dqkv) || misaligned(workspace) || misaligned(fwd_mask, 3) ||
      misaligned(key_len, 3))
    return TS_EUNSUPPORTED;
  // the dynamic-LDS limit of the dKV kernel, once per device
  static bool attr[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return TS_EINVAL;
  if (!attr[dev]) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(mt_bwd_dkv_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)MT_DKV_LDS) != hipSuccess)
      return TS_EUNSUPPORTED;
    attr[dev] = true;
  }
  TS_STREAM;
  MtArgs a = mt_args(qkv_bf16, t, c, heads, key_len, p_drop);
  a.lse2 = const_cast<float*>(lse2); a.dqkv = dqkv;
  unsigned short* const dout16 = static_cast<unsigned short*>(workspace);
  float* const dsum = reinterpret_cast<float*>(static_cast<char*>(workspace) + al16((int64_t)batch * t * c * 2));
  a.dout = dout16; a.dsum = dsum;
  if (p_drop > 0.f && fwd_mask) a.mask = static_cast<const unsigned*>(fwd_mask);      // the forward's workspace, kept by the caller
  else if (p_drop > 0.f) {                                                            // or re-drawn: the mask is a pure function of the seed
    unsigned* const mask = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(dsum) + al16((int64_t)batch * heads * t * 4));
    attn_draw_mask(mask, batch, t, heads, seed, p_drop, stream);
    a.mask = mask;
  }
  const long long units = (long long)batch * t * heads;
  hipLaunchKernelGGL(mt_rowdot_kernel, dim3((unsigned)((units + 63) / 64)), dim3(256), 0, stream, dctx, ctx, dout16, dsum, units, t, c, heads);
  hipLaunchKernelGGL(mt_bwd_dq_kernel, dim3((t + AT_QW - 1) / AT_QW, heads, batch), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(mt_bwd_dkv_kernel, dim3((t + AT_KT - 1) / AT_KT, heads, batch), dim3(256), MT_DKV_LDS, stream, a);
  return hip_status(hipGetLastError());
}
