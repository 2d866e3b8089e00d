// The tile code shared by the fused (flash-style) attention kernels: w2v_flash_attn_kernel<HD> (csrc/w2v_attn.hip) and attn_fwd_train_kernel<HD> /
// attn_bwd_dq_kernel<HD> / attn_bwd_dkv_kernel<HD> (csrc/w2v_attn_train.hip), each instantiated for head_dim 64 (wav2vec2) and 80 (XLS-R 1B / MMS:
// ts_mms_attention_fwd in csrc/mms.hip, ts_mms_attention_train_* in csrc/mms_train.hip), and the head_dim 64 kernels with WavLM's gated bias:
// wavlm_flash_attn_kernel (csrc/wavlm.hip), wt_fwd_kernel / wt_bwd_dq_kernel / wt_bwd_dkv_kernel (csrc/wavlm_train.hip).  Each kernel is a
// sequence of these helpers plus what is its own.  The helpers take the head dimension HD, or the array extents that follow from it (k-steps HD / 16,
// 32-row d blocks (HD + 31) / 32), and the pitch of each staged tile as template parameters that default to the head_dim 64 values.
//
//   workgroup = 128 queries of one (clip, head), 4 waves x 32 queries; K / V tiles of 64 keys staged in LDS for all 4 waves.
//   Per 32-key sub-tile and wave, v_mfma_f32_32x32x16_bf16 throughout:
//     S^T[key][query] = K Q^T   -- transposed on purpose: a lane then owns ONE query column and 16 of the 32 keys, so the
//                                  row maximum / sum of the online softmax are in-lane plus one exchange with lane ^ 32;
//     O^T[d][query] += V^T P^T  -- A = V^T read out of the [key][d] tile with ds_read_b64_tr_b16, B = P^T straight from
//                                  the accumulator registers of the first product: the K rows are loaded in the order
//                                  (bits 2 and 3 of the row index swapped) that makes accumulator register i of lane half h
//                                  hold key 16 (i / 8) + 8 h + i % 8, which is exactly the B-operand slot order.
//   Probabilities are rounded to bf16 for the second product (as in the unfused path), everything else is fp32.
//   The backward's dQ kernel is the same loop with dS in place of P and K in place of V; its dKV kernel turns the roles round (workgroup = 64 keys,
//   loop over query tiles) and passes P and dS through wave-private LDS tiles.
// The last section holds what only the four WavLM kernels use: the gate and the staged window of position-bias diagonals.
//
// The score tile and the running softmax state go through the forward helpers BY VALUE (s = f(s, ...)), and the dKV kernels keep the MFMAs on their
// 128 accumulators in the kernel body: a local whose address is passed to a helper stays in memory form until the helper is inlined, and the
// register allocation that comes out differs (measured: +32 bytes of scratch in wt_fwd_kernel, 264 -> 280 VGPRs in attn_bwd_dkv_kernel<64>).
#pragma once
#include "ts_common.hpp"

namespace ts {

constexpr int AT_KT = 64;                      // keys per staged tile
constexpr int AT_PITCH = 144;                  // bytes per staged row: 64 bf16 + 16 (rows 36 banks apart: conflict-free b128 / tr reads)
constexpr int AT_QW = 128;                     // queries per workgroup of the forward / dQ kernels (4 waves x 32)
constexpr int AT_KV = AT_KT * AT_PITCH;        // one staged K or V tile
constexpr int AT_WTILE = 32 * AT_PITCH;        // one wave's [32 rows][64 columns] bf16 tile
constexpr size_t AT_DKV_LDS = (size_t)2 * AT_KV + (size_t)4 * 4 * AT_WTILE;   // head_dim 64 dKV kernels: K, V + 4 waves x 4 tiles (72 KiB; one round of the final sums needs 64)
constexpr float LOG2E = 1.4426950408889634f;

// Geometry by head dimension.  A first product (S^T = K Q^T, dP^T = V dO^T) takes HD / 16 k-steps and reads its tile by rows (ds_read_b128); a second
// product (O^T += V^T P^T, dQ^T += K^T dS^T, dV^T += dO^T Pd, dK^T += Q^T dS) covers d in (HD + 31) / 32 blocks of 32 rows and reads its tile transposed
// (ds_read_b64_tr_b16).  At head_dim 80 rows 80..95 of the third block belong to no output: an MFMA A row feeds only its own output row, so those columns
// of a tile only have to be legal to read.  Every tile that is read transposed is 96 columns wide or wider, its pad columns 80..95 are zeroed once
// (zero_pad), and every epilogue stores d < 80 only (head h's columns end where head h + 1's begin).
//
// LDS pitches in bytes: RP of a tile read by rows only, TP read transposed only, BP read both ways.  Head_dim 64 takes AT_PITCH for all three.  Head_dim
// 80, by the bank rules (bank = dword address mod 64; a b128 read is served per 16-lane group, which reads rows of all 16 residues mod 16 at one
// column; a transposing b64 read per 32-lane half, which reads 4 rows x 16 consecutive dwords, and once more 4 rows further down):
//   RP (forward K; dQ kernel V; dKV kernel K and V):  176 bytes = 44 dwords.  44 r mod 64 = 4 (11 r mod 16) puts the 16 rows on 16 different 4-dword
//     slots: conflict-free (any pitch of 4 x odd dwords does it; 44 is the smallest over 40).
//   TP (forward V):  192 bytes = 48 dwords, the 96 columns and no pad: the four rows start at banks 0, 48, 32, 16, a quarter of the banks each:
//     conflict-free.
//   BP (dQ kernel K; dKV kernel's wave-private Q and dO tiles):  no pitch serves both.  The b128 rule needs pitch = 4 x odd dwords, i.e. pitch mod 16
//     in {4, 12}.  The transposing read needs the 16-bank windows that start at 0, P, 2P, 3P (mod 64) disjoint; four windows of 16 on a ring of 64 are
//     disjoint only when they tile it, P mod 64 in {16, 48} -- a multiple of 16, never 4 x odd.  These tiles take 208 bytes = 52 dwords (the smallest
//     4 x odd pitch that holds 96 columns): the b128 row reads are conflict-free, and the TRANSPOSING read pays: its windows start at banks 0, 52, 40, 28,
//     so neighbouring rows overlap on 4 banks each (0-3, 52-55, 40-43): 12 of the 64 banks are hit two ways, the other 52 once.  The other choice, 192
//     bytes, would make every b128 read four ways (48 r mod 64 takes 4 values over 16 rows); a sub-tile issues 10 b128 and 12 transposing reads.
//   The dKV kernel's Pd / dS tiles (written as b128 rows, read transposed, 64 columns) take AT_PITCH at either head dimension.
// DKV_RED: where the dKV kernel's final sums start in its allocation -- behind K and V (64), over the whole allocation (80: 96 KiB a round).
// FWD_TRAIN_WAVES: the training forward's amdgpu_waves_per_eu (csrc/w2v_attn_train.hip says why they differ).
template <int HD> struct AttnGeom;
template <> struct AttnGeom<64> { static constexpr int RP = AT_PITCH, TP = AT_PITCH, BP = AT_PITCH, DKV_RED = 2 * AT_KV, FWD_TRAIN_WAVES = 4; };
template <> struct AttnGeom<80> { static constexpr int RP = 176, TP = 192, BP = 208, DKV_RED = 0, FWD_TRAIN_WAVES = 3; };
// dKV kernels: K, V (rows only) + per wave Q | dO (32 rows, both ways) | Pd | dS (32 rows, AT_PITCH): 90 KiB / 110 KiB
template <int HD> constexpr size_t at_dkv_lds() { return (size_t)2 * AT_KT * AttnGeom<HD>::RP + (size_t)4 * (2 * 32 * AttnGeom<HD>::BP + 2 * AT_WTILE); }
static_assert(at_dkv_lds<64>() == AT_DKV_LDS, "head_dim 64 keeps its allocation");

// ---- host pieces of the training paths, defined once in csrc/w2v_attn_train.hip ----
inline int64_t al16(int64_t n) { return (n + 15) / 16 * 16; }
int attn_train_check(const void* qkv, int32_t batch, int32_t t, int32_t c, int32_t heads, float p_drop);
long long attn_mask_words(int batch, int t, int heads);
void attn_draw_mask(unsigned* mask, int batch, int t, int heads, unsigned long long seed, float p, hipStream_t stream);
void attn_rowdot(const float* dctx, const float* ctx, unsigned short* dout16, float* dsum, int batch, int t, int c, int heads, hipStream_t stream);
// What ts_w2v_attention_train_* (hd 64) and ts_mms_attention_train_* (hd 80) do once their own argument checks have passed, and their workspace sizes
// (forward: the mask bits; backward: dO bf16 [B][t][c] | D f32 [B][H][t] | the mask bits, used when fwd_mask is NULL and p_drop > 0)
int64_t attn_train_fwd_workspace(int32_t batch, int32_t t, int32_t c, int32_t heads);
int64_t attn_train_bwd_workspace(int32_t batch, int32_t t, int32_t c, int32_t heads);
int attn_train_fwd_launch(int hd, const void* qkv_bf16, int32_t batch, int32_t t, int32_t c, int32_t heads, const int32_t* key_len, float p_drop, uint64_t seed,
                          float* ctx, float* lse2, void* workspace, hipStream_t stream);
int attn_train_bwd_launch(int hd, const void* qkv_bf16, int32_t batch, int32_t t, int32_t c, int32_t heads, const int32_t* key_len, float p_drop, uint64_t seed,
                          const float* dctx, const float* ctx, const float* lse2, const void* fwd_mask, float* dqkv, void* workspace, hipStream_t stream);
// the fused inference core (bf16 in, bf16 out) of ts_w2v_attention_fwd (hd 64) and ts_mms_attention_fwd (hd 80), defined in csrc/w2v_attn.hip
int attn_flash_launch(int hd, const void* qkv, int32_t batch, int32_t t, int32_t c, int32_t heads, const int32_t* key_len, void* ctx, hipStream_t stream);

// number of keys a clip attends to.  No valid key: ALL_IF_EMPTY -- the reference's softmax degenerates to all keys (inference, as ts_w2v_attention_fwd);
// otherwise none -- every probability 0, ctx = 0 (the training convention, as ts_w2v_softmax_fwd)
template <bool ALL_IF_EMPTY>
__device__ __forceinline__ int key_limit(const int* key_len, int b, int t) {
  int lim = t;
  if (key_len) {
    const int n = key_len[b] < t ? key_len[b] : t;
    lim = n > 0 ? n : (ALL_IF_EMPTY ? t : 0);
  }
  return lim;
}

// K and V rows k0 .. k0 + 63 of one (clip, head) into LDS at pitches KP / VP, HD / 8 chunks of 16 bytes per row: 512 or 640 chunks for 256 threads
// (rows past t clamped to t - 1: never stored, their probabilities are 0)
template <int HD = 64, int KP = AT_PITCH, int VP = KP>
__device__ __forceinline__ void stage_kv(char* ks_, char* vs_, const unsigned short* base, size_t rowp, int c, int t, int k0, int tid) {
  constexpr int CPR = HD / 8, CHUNKS = AT_KT * CPR;
#pragma unroll
  for (int rep = 0; rep < (CHUNKS + 255) / 256; ++rep) {
    const int chunk = tid + 256 * rep;
    if (CHUNKS % 256 == 0 || chunk < CHUNKS) {
      const int r = chunk / CPR, cc = chunk - CPR * r;
      const int key = k0 + r < t ? k0 + r : t - 1;
      const unsigned short* src = base + (size_t)key * rowp + cc * 8;
      *reinterpret_cast<uint4*>(ks_ + r * KP + cc * 16) = *reinterpret_cast<const uint4*>(src + c);
      *reinterpret_cast<uint4*>(vs_ + r * VP + cc * 16) = *reinterpret_cast<const uint4*>(src + 2 * c);
    }
  }
}

// the pad columns HD .. 32 blocks - 1 of `rows` tile rows at pitch P, by `n` threads (idx = this one); nothing when HD is a multiple of 32
template <int HD, int P>
__device__ __forceinline__ void zero_pad(char* tile, int rows, int idx, int n) {
  constexpr int PAD = (HD + 31) / 32 * 4 - HD / 8;                              // 16-byte chunks per row
  if constexpr (PAD > 0)
    for (int i = idx; i < PAD * rows; i += n) *reinterpret_cast<uint4*>(tile + (i / PAD) * P + (HD / 8 + i % PAD) * 16) = uint4{0u, 0u, 0u, 0u};
}

struct TileLane {
  int half, n32;     // k-half of the MFMA operands, column (query, or key in the dKV contraction) within the wave's 32
  int pm;            // K / V row this lane loads as A operand: n32 with bits 2 and 3 swapped (why: the top of this file)
  int tr_off;        // transposing read of a staged tile of pitch P: rows = contraction index, columns = M index
};
template <int P = AT_PITCH>
__device__ __forceinline__ TileLane tile_lane(int lane) {
  const int half = lane >> 5, n32 = lane & 31;
  const int pm = (n32 & ~12) | ((n32 & 4) << 1) | ((n32 & 8) >> 1);
  const int q4 = (lane >> 2) & 3, gq = (lane >> 4) & 1, p4 = lane & 3;
  return TileLane{half, n32, pm, (8 * half + q4) * P + (16 * gq + 4 * p4) * 2};
}

__device__ __forceinline__ void zero(f32x16& v) {
#pragma unroll
  for (int i = 0; i < 16; ++i) v[i] = 0.f;
}

// B operand of the first products, lane = (query n32, k-half): 8 consecutive d per k-step, from the row's HD = 16 KS bf16 at p = row + 8 half
template <int KS>
__device__ __forceinline__ void load_row_frags(s16x8 (&f)[KS], const unsigned short* p) {
  const uint4* p4 = reinterpret_cast<const uint4*>(p);
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) f[ks] = __builtin_bit_cast(s16x8, p4[2 * ks]);
}

// S^T = K Q^T of 32-key sub-tile `sub`; accumulator register i <-> key k0 + 32 sub + 16 (i / 8) + 8 half + i % 8 (the order mask_tail / bwd_tile expect)
template <int P = AT_PITCH, int KS>
__device__ __forceinline__ f32x16 qk_subtile(const char* ks_, int sub, const TileLane& g, const s16x8 (&qf)[KS]) {
  f32x16 s;
  zero(s);
  const char* kr = ks_ + (sub * 32 + g.pm) * P + g.half * 16;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const s16x8*>(kr + ks * 32), qf[ks], s, 0, 0, 0);
  return s;
}

// the backward's pair: S^T = K Q^T and dP^T = V dO^T, same register <-> key mapping.  At four k-steps (head_dim 64) the two chains are interleaved, at
// five (80) one follows the other: the orders in which the kernels of either head dimension were written, and the compiler's schedule follows the
// source.  Measured in the other's order, attn_bwd_dq_kernel<80> was 2 % slower interleaved and attn_bwd_dq_kernel<64> 0.9 % slower as two chains
// (profiles/attention_head_dim_refactor.md).
template <int KP = AT_PITCH, int VP = KP, int KS>
__device__ __forceinline__ void qk_dp_subtile(f32x16& s, f32x16& dp, const char* ks_, const char* vs_, int sub, const TileLane& g, const s16x8 (&qf)[KS],
                                              const s16x8 (&gf)[KS]) {
  if constexpr (KS != 4) {
    s = qk_subtile<KP>(ks_, sub, g, qf);
    dp = qk_subtile<VP>(vs_, sub, g, gf);
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) { s[i] = 0.f; dp[i] = 0.f; }
    const char* kr = ks_ + (sub * 32 + g.pm) * KP + g.half * 16;
    const char* vr = vs_ + (sub * 32 + g.pm) * VP + g.half * 16;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const s16x8*>(kr + ks * 32), qf[ks], s, 0, 0, 0);
      dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const s16x8*>(vr + ks * 32), gf[ks], dp, 0, 0, 0);
    }
  }
}

// keys past lim get probability 0; kbase = k0 + 32 sub + 8 half
__device__ __forceinline__ f32x16 mask_tail(f32x16 s, int kbase, int lim) {
#pragma unroll
  for (int i = 0; i < 16; ++i)
    if (kbase + 16 * (i >> 3) + (i & 7) >= lim) s[i] = -INFINITY;
  return s;
}

// one step of the online softmax over the lane's 16 keys (+ the 16 of lane ^ 32): p = exp2(logit - new maximum), alpha = the factor the running
// output is to be scaled by, m / l = the new running maximum / normaliser.  SCALED: s holds raw q . k and the scale (> 0: the maximum commutes with
// it) is folded into the exponent's fma; otherwise s already holds the logit in log2 units and no scale is passed.  The maximum is finite: the first sub-tile holds key 0.
// Bare v_exp_f32 (exp2): the arguments are <= 0 and a flushed denormal is a zero weight -- the library form's range handling
// (compare, scale, select around every exp) was a third of this VALU-bound loop's instructions.
struct SoftmaxStep { f32x16 p; float alpha, m, l; };
template <bool SCALED>
__device__ __forceinline__ SoftmaxStep softmax_step(f32x16 s, float m_run, float l_run, float scale_log2e = 1.f) {
  float mx = s[0];
#pragma unroll
  for (int i = 1; i < 16; ++i) mx = fmaxf(mx, s[i]);
  mx = fmaxf(mx, __shfl_xor(mx, 32));
  const float m_new = fmaxf(m_run, SCALED ? mx * scale_log2e : mx);
  const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
  float rs = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) { s[i] = __builtin_amdgcn_exp2f(SCALED ? fmaf(s[i], scale_log2e, -m_new) : s[i] - m_new); rs += s[i]; }
  return SoftmaxStep{s, alpha, m_new, l_run * alpha + rs};                    // the normaliser counts every key, dropped or not
}

template <int DB>
__device__ __forceinline__ void rescale(f32x16 (&o)[DB], float alpha) {
  if (__any(alpha != 1.f)) {                                                  // after the first tiles the running maximum rarely moves
#pragma unroll
    for (int mt = 0; mt < DB; ++mt)
#pragma unroll
      for (int i = 0; i < 16; ++i) o[mt][i] *= alpha;
  }
}

// two ds_read_b64_tr_b16: the 8 operand elements of one k-step of 16 rows, transposed out of a row-major tile of pitch P
template <int P = AT_PITCH>
__device__ __forceinline__ s16x8 tr8(const char* p) {
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((TS_LDS s16x4*)((TS_LDS char*)p));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((TS_LDS s16x4*)((TS_LDS char*)p + 4 * P));
  return s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// acc^T[d][query] += tile^T x^T over the 32 keys of sub-tile `sub`: x (P, or dS) goes from the accumulators to the bf16 B operand, the staged
// [key][d] tile (V, or K; pitch P, g = tile_lane<P>) is read transposed; acc[mt] holds d = 32 mt .. 32 mt + 31 (d >= HD: the zeroed pad columns)
template <int P = AT_PITCH, int DB>
__device__ __forceinline__ void acc_tile_t(f32x16 (&acc)[DB], const f32x16& x, const char* tile, int sub, const TileLane& g) {
#pragma unroll
  for (int ks2 = 0; ks2 < 2; ++ks2) {
    const unsigned p01 = pack_bf16(x[8 * ks2 + 0], x[8 * ks2 + 1]), p23 = pack_bf16(x[8 * ks2 + 2], x[8 * ks2 + 3]);
    const unsigned p45 = pack_bf16(x[8 * ks2 + 4], x[8 * ks2 + 5]), p67 = pack_bf16(x[8 * ks2 + 6], x[8 * ks2 + 7]);
    const s16x8 pb = __builtin_bit_cast(s16x8, uint4{p01, p23, p45, p67});
#pragma unroll
    for (int mt = 0; mt < DB; ++mt)
      acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr8<P>(tile + (sub * 32 + 16 * ks2) * P + g.tr_off + 64 * mt), pb, acc[mt], 0, 0, 0);
  }
}

// epilogues of the forward / dQ kernels, dst = the lane's output row + HD head + 4 half: accumulator registers 4g .. 4g+3 <-> d = 32 mt + 8 g + 4 half + 0..3;
// the last block stops at d = HD
template <int HD = 64>
__device__ __forceinline__ void store_bf16(unsigned short* dst, const f32x16 (&o)[(HD + 31) / 32], float mul) {
#pragma unroll
  for (int mt = 0; mt < (HD + 31) / 32; ++mt)
#pragma unroll
    for (int g = 0; g < 4 && 32 * mt + 8 * g < HD; ++g)
      *reinterpret_cast<uint2*>(dst + 32 * mt + 8 * g) =
          uint2{pack_bf16(o[mt][4 * g] * mul, o[mt][4 * g + 1] * mul), pack_bf16(o[mt][4 * g + 2] * mul, o[mt][4 * g + 3] * mul)};
}
template <int HD = 64>
__device__ __forceinline__ void store_f32(float* dst, const f32x16 (&o)[(HD + 31) / 32], float mul) {
#pragma unroll
  for (int mt = 0; mt < (HD + 31) / 32; ++mt)
#pragma unroll
    for (int g = 0; g < 4 && 32 * mt + 8 * g < HD; ++g)
      *reinterpret_cast<f32x4*>(dst + 32 * mt + 8 * g) = f32x4{o[mt][4 * g] * mul, o[mt][4 * g + 1] * mul, o[mt][4 * g + 2] * mul, o[mt][4 * g + 3] * mul};
}

// first element of a query's row in the logical [B * heads * T][T] dropout stream
__device__ __forceinline__ unsigned long long mask_row(int b, int heads, int head, int t, int qrow) {
  return (((unsigned long long)b * heads + head) * t + qrow) * (unsigned long long)t;
}

// ---------------------------------------------------------------------------------------------------------------------
// training: dropout keep bits and the backward's tile arithmetic
// ---------------------------------------------------------------------------------------------------------------------
// keep bits of the 8 consecutive elements e0 .. e0 + 7 (bit j: element e0 + j is kept) of the mask bitstring (attn_mask_kernel)
__device__ __forceinline__ unsigned keep8(const unsigned* __restrict__ mask, unsigned long long e0) {
  const unsigned long long w = e0 >> 5;
  const unsigned long long both = ((unsigned long long)mask[w + 1] << 32) | mask[w];
  return (unsigned)(both >> (e0 & 31)) & 0xffu;
}

// forward: dropout on the lane's 16 probabilities, e0 = element of (query, key kbase)
__device__ __forceinline__ f32x16 drop_keys(f32x16 s, const unsigned* __restrict__ mask, unsigned long long e0, float keep_scale) {
  const unsigned k_lo = keep8(mask, e0), k_hi = keep8(mask, e0 + 16);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    s[i] = (k_lo >> i) & 1u ? s[i] * keep_scale : 0.f;
    s[8 + i] = (k_hi >> i) & 1u ? s[8 + i] * keep_scale : 0.f;
  }
  return s;
}

// backward: probabilities, mask and dS of one 32-key sub-tile; registers i <-> key kbase + 16 (i / 8) + i % 8, lane <-> one query
//   in:  s = q . k (raw), dp = dO . v (raw);  out: s = P * keep / (1 - p) (the dV operand), dp = dS = P * (dP - D)
// BIAS: the logit is s scale + gl wr[16 (i / 8) + i % 8] (wr = the staged bias diagonals of (query, key), gl = the query's gate in log2 units);
// without it the two are not passed
template <bool BIAS>
__device__ __forceinline__ void bwd_tile(f32x16& s, f32x16& dp, int kbase, int lim, bool q_ok, float lse2, float dsum, float scale_log2e, float keep_scale,
                                         const unsigned* __restrict__ mask, unsigned long long erow, bool drop, const float* wr = nullptr, float gl = 0.f) {
  unsigned k_lo = 0xffu, k_hi = 0xffu;
  if (drop) { k_lo = keep8(mask, erow + kbase); k_hi = keep8(mask, erow + kbase + 16); }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int key = kbase + 16 * (i >> 3) + (i & 7);
    float p;
    if constexpr (BIAS) {
      const float z = fmaf(s[i], scale_log2e, gl * wr[16 * (i >> 3) + (i & 7)]);
      p = (q_ok && key < lim) ? __builtin_amdgcn_exp2f(z - lse2) : 0.f;
    } else {
      p = (q_ok && key < lim) ? __builtin_amdgcn_exp2f(fmaf(s[i], scale_log2e, -lse2)) : 0.f;
    }
    const bool kept = (((i < 8 ? k_lo : k_hi) >> (i & 7)) & 1u) != 0;
    const float ks = kept ? keep_scale : 0.f;
    const float dpv = dp[i] * ks;
    dp[i] = p * (dpv - dsum);
    s[i] = p * ks;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// dKV kernels: workgroup = 64 keys of one (clip, head), loop over 128-query tiles (32 per wave).  Per wave and tile the Q and dO rows are staged in
// wave-private LDS (wt: Q | dO, 32 rows at pitch QP each, then Pd | dS, AT_WTILE each), P * keep / (1 - p) and dS go there as bf16 [query][key] tiles, and
//   dV^T[d][key] += dO^T[d][q] Pd[q][key],   dK^T[d][key] += Q^T[d][q] dS[q][key]
// take both operands out of those tiles with transposing reads (contraction over the tile's 32 queries); the four waves' sums meet in LDS at the end.
// The tiles are wave-private: LDS operations of a wave execute in order, so an s_waitcnt + wave_barrier pair between the phases is all the
// synchronisation the loop needs (the kernels keep those pairs themselves).
// ---------------------------------------------------------------------------------------------------------------------
// the wave's 32 Q and dO rows, HD / 8 chunks of 16 bytes each (rows past t clamped to t - 1: q_ok zeroes their probabilities)
template <int HD = 64, int QP = AT_PITCH>
__device__ __forceinline__ void dkv_stage_rows(char* wt, const unsigned short* base, size_t rowp, const unsigned short* dout, int b, int head, int t, int c,
                                               int q0, int lane) {
  constexpr int CPR = HD / 8;
#pragma unroll
  for (int rep = 0; rep < CPR / 2; ++rep) {
    const int chunk = lane + 64 * rep, r = chunk / CPR, cc = chunk - CPR * r;
    const int qr = q0 + r < t ? q0 + r : t - 1;
    *reinterpret_cast<uint4*>(wt + r * QP + cc * 16) = *reinterpret_cast<const uint4*>(base + (size_t)qr * rowp + cc * 8);
    *reinterpret_cast<uint4*>(wt + 32 * QP + r * QP + cc * 16) =
        *reinterpret_cast<const uint4*>(dout + ((size_t)b * t + qr) * c + (size_t)head * HD + cc * 8);
  }
}

template <int QP = AT_PITCH, int KS>
__device__ __forceinline__ void dkv_load_frags(s16x8 (&qf)[KS], s16x8 (&gf)[KS], const char* wt, const TileLane& g) {
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    qf[ks] = *reinterpret_cast<const s16x8*>(wt + g.n32 * QP + (16 * ks + 8 * g.half) * 2);
    gf[ks] = *reinterpret_cast<const s16x8*>(wt + 32 * QP + g.n32 * QP + (16 * ks + 8 * g.half) * 2);
  }
}

// Pd (s) and dS (dp) of sub-tile `sub` into the wave's tiles: row = this lane's query, columns = the keys of its two runs of 8: 32 sub + 8 half + 0..7 and + 16
template <int QP = AT_PITCH>
__device__ __forceinline__ void dkv_store_tiles(char* wt, const f32x16& s, const f32x16& dp, int sub, const TileLane& g) {
  char* const pt = wt + 2 * 32 * QP;
  char* const st = pt + AT_WTILE;
#pragma unroll
  for (int run = 0; run < 2; ++run) {
    const int col = (32 * sub + 16 * run + 8 * g.half) * 2;
    *reinterpret_cast<uint4*>(pt + g.n32 * AT_PITCH + col) = uint4{pack_bf16(s[8 * run + 0], s[8 * run + 1]), pack_bf16(s[8 * run + 2], s[8 * run + 3]),
                                                                    pack_bf16(s[8 * run + 4], s[8 * run + 5]), pack_bf16(s[8 * run + 6], s[8 * run + 7])};
    *reinterpret_cast<uint4*>(st + g.n32 * AT_PITCH + col) = uint4{pack_bf16(dp[8 * run + 0], dp[8 * run + 1]), pack_bf16(dp[8 * run + 2], dp[8 * run + 3]),
                                                                    pack_bf16(dp[8 * run + 4], dp[8 * run + 5]), pack_bf16(dp[8 * run + 6], dp[8 * run + 7])};
  }
}

// contraction over the tile's 32 queries, k-step ks of 16: the A operands dO^T (ga), Q^T (qa), DB 32-column blocks each, and the B operands Pd (pb),
// dS (sb), two each, for dv[mt][nt] += ga[mt] pb[nt], dk[mt][nt] += qa[mt] sb[nt].  tr_q = tile_lane<QP>'s tr_off; g.tr_off is the Pd / dS tiles'
template <int QP = AT_PITCH, int DB>
__device__ __forceinline__ void dkv_operands(s16x8 (&ga)[DB], s16x8 (&qa)[DB], s16x8 (&pb)[2], s16x8 (&sb)[2], const char* wt, int ks, const TileLane& g,
                                             int tr_q) {
#pragma unroll
  for (int x = 0; x < DB; ++x) {
    const int off = 16 * ks * QP + tr_q + 64 * x;
    ga[x] = tr8<QP>(wt + 32 * QP + off); qa[x] = tr8<QP>(wt + off);
  }
#pragma unroll
  for (int x = 0; x < 2; ++x) {
    const int off = 2 * 32 * QP + 16 * ks * AT_PITCH + g.tr_off + 64 * x;
    pb[x] = tr8(wt + off); sb[x] = tr8(wt + AT_WTILE + off);
  }
}

// the four waves' sums: red = [wave][block = 2 mt + nt][16][64 lanes] f32 over the (now idle) tiles, NB = 2 d blocks x 2 key blocks per wave -- 64 or
// 96 KiB a round, so in two rounds (dv, then dk scaled); wave w finishes blocks w, w + 4, .. < NB and writes them to dqkv's V (K) third; the last d block
// stops at HD.  Call after a __syncthreads().  The store test is written per block and group (mt < HD / 32 || gg < HD % 32 / 8), not as
// 32 mt + 8 gg < HD: the second form put every store of the head_dim 80 kernel behind its own exec mask and spread the LDS reads of the sums over them.
template <int HD = 64>
__device__ __forceinline__ void dkv_reduce_store(float* red, const f32x16 (&dv)[(HD + 31) / 32][2], const f32x16 (&dk)[(HD + 31) / 32][2], float scale,
                                                 float* dqkv, size_t rowp, int b, int t, int c, int head, int k0, int wave, int lane, const TileLane& g) {
  constexpr int NB = 2 * ((HD + 31) / 32), WSTRIDE = NB * 16 * 64;             // a wave's partial sums
#pragma unroll
  for (int which = 0; which < 2; ++which) {
#pragma unroll
    for (int mt = 0; mt < NB / 2; ++mt)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int i = 0; i < 16; ++i) red[(((size_t)wave * NB + mt * 2 + nt) * 16 + i) * 64 + lane] = which ? dk[mt][nt][i] : dv[mt][nt][i];
    __syncthreads();
    for (int blk = wave; blk < (NB % 4 == 0 ? wave + NB : NB); blk += 4) {         // NB % 4 == 0: NB / 4 blocks for every wave, a constant trip count
      const int mt = blk >> 1, nt = blk & 1;
      f32x16 tot;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        // waves 0, 1, 2, 3 in this order, pinned: -ffast-math lets the compiler reassociate the sum, it chooses by context, and the bits of
        // dK and dV depend on the choice
#pragma clang fp reassociate(off)
        const float* part = red + ((size_t)blk * 16 + i) * 64 + lane;              // wave w's partial sum: part[w * WSTRIDE]
        const float v = ((part[0] + part[1 * WSTRIDE]) + part[2 * WSTRIDE]) + part[3 * WSTRIDE];
        tot[i] = which ? v * scale : v;
      }
      // accumulator register r of block (mt, nt): d = 32 mt + (r & 3) + 8 (r >> 2) + 4 half, key = k0 + 32 nt + n32
      const int key = k0 + 32 * nt + g.n32;
      if (key < t) {
        float* dst = dqkv + ((size_t)b * t + key) * rowp + (size_t)(which ? 1 : 2) * c + (size_t)head * HD + 32 * mt + 4 * g.half;
#pragma unroll
        for (int gg = 0; gg < 4; ++gg)
          if (HD % 32 == 0 || mt < HD / 32 || gg < HD % 32 / 8) *reinterpret_cast<f32x4*>(dst + 8 * gg) = f32x4{tot[4 * gg], tot[4 * gg + 1], tot[4 * gg + 2], tot[4 * gg + 3]};
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// WavLM: the gate and the position bias.  The logit is s scale + gate[query] rb[h][key - query + t - 1]; a tile touches one window of consecutive
// diagonals, staged in LDS next to K and V.  With a bias the maximum no longer commutes with the scale, so the full logit (log2 units) is formed
// BEFORE the running maximum: softmax_step<false>.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int AT_WIN = AT_QW + AT_KT;          // 191 diagonals of a 128 x 64 tile, rounded up

__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + __expf(-x)); }

// gate = sigmoid(p0 + p1 + p2 + p3) (sigmoid(p4 + p5 + p6 + p7) const - 1) + 2 from the 8 projections p (bias included)
__device__ __forceinline__ float wavlm_gate(const float* p, float cst) {
  const float a = sigmoid_f(((p[0] + p[1]) + p[2]) + p[3]);
  const float g = sigmoid_f(((p[4] + p[5]) + p[6]) + p[7]);
  return a * (g * cst - 1.f) + 2.f;
}

// embedding row of diagonal d = key - query (the bucket table is built on the host); clamped: a malformed table cannot reach outside E
__device__ __forceinline__ int wavlm_bucket(int d, int nb, int md, const int* __restrict__ abs_bucket) {
  const int ad = d < 0 ? -d : d;
  const int bucket = (d > 0 ? nb / 2 : 0) + abs_bucket[ad < md ? ad : md];
  return bucket < 0 ? 0 : (bucket < nb ? bucket : nb - 1);
}

// rb[h][d + t - 1] (diagonals outside [-(t - 1), t - 1] clamped: they belong to clamped keys / queries, never stored)
__device__ __forceinline__ float rb_at(const float* rbh, int t, int d) {
  int j = d + t - 1;
  j = j < 0 ? 0 : (j > 2 * t - 2 ? 2 * t - 2 : j);
  return rbh[j];
}

// the forward / dQ kernels' window of key tile k0, query tile qw0: slot of (key k0 + kk, query qw0 + qq) is kk - qq + AT_QW - 1
__device__ __forceinline__ void stage_window(float* rbs, const float* rbh, int t, int k0, int qw0, int tid) {
  if (tid < AT_WIN) rbs[tid] = rb_at(rbh, t, k0 - qw0 - (AT_QW - 1) + tid);
}
// the lane's first slot in it (sub-tile 0): its query is qq = 32 wave + n32, its keys start at 8 half
__device__ __forceinline__ int window_base(int wave, const TileLane& g) { return AT_QW - 1 - (wave * 32 + g.n32) + 8 * g.half; }

// s = q . k  ->  the logit in log2 units, wr = the lane's window slots of this sub-tile
__device__ __forceinline__ f32x16 wavlm_logits(f32x16 s, float scale_log2e, float gl, const float* wr) {
#pragma unroll
  for (int i = 0; i < 16; ++i) s[i] = fmaf(s[i], scale_log2e, gl * wr[16 * (i >> 3) + (i & 7)]);
  return s;
}

}  // namespace ts
