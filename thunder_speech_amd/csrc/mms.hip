// What MMS (facebook/mms-1b-*) and XLS-R 1B need beyond the wav2vec2 launches (include/thunder_speech_amd_mms.h):
//   ts_mms_attention_fwd     the fused attention core at head_dim 80 (hidden 1280, 16 heads): mms_flash_attn_kernel
//   ts_mms_attn_adapter_fwd  h += W2 relu(W1 LN(h) + b1) + b2 in place on the residual stream, with the LayerNorm that follows it: mms_adapter_kernel
// adapter_launch (declared in mms_adapter_rows.hpp) is that kernel's launcher, also used by ts_mms_attn_adapter_train_fwd (csrc/mms_adapter_train.hip).
#include "attn_tile.hpp"
#include "mms_adapter_rows.hpp"
#include "thunder_speech_amd_mms.h"

namespace ts {

// ---------------------------------------------------------------------------------------------------------------------
// Fused attention, head_dim 80.  The scheme is w2v_flash_attn_kernel's (csrc/attn_tile.hpp describes it): 128 queries per workgroup as 4 waves x 32,
// K / V tiles of 64 keys in LDS, S^T = K Q^T and O^T += V^T P^T on v_mfma_f32_32x32x16_bf16, the online softmax with the scale in the exponent.
// From attn_tile.hpp come the pieces that do not know the head dimension (key_limit, tile_lane's lane mapping, mask_tail, softmax_step, zero);
// the tile helpers below are this kernel's own -- the head_dim-64 ones are not templated, their kernels' register allocation moves with their shape.
//   S^T: five k-steps (80 = 5 x 16).   O^T: three 32-row blocks of d, 0..95.  Rows 80..95 of the third belong to no output: an MFMA A row
//   feeds only its own output row, so they only have to be legal to read -- the staged V rows are 96 columns wide, the pad is zeroed once, and
//   the epilogue stores d < 80 only (head h's columns end where head h + 1's begin).
// LDS pitches, by the bank rules of the b128 and the transposing b64 reads (bank = dword address mod 64):
//   K, read with ds_read_b128 only: 176 bytes = 44 dwords.  A 16-lane group reads rows of all 16 residues mod 16 at one column; 44 r mod 64 =
//     4 (11 r mod 16) puts them on 16 different 4-dword slots: conflict-free (any pitch of 4 x odd dwords does it; 44 is the smallest over 40).
//   V, read with ds_read_b64_tr_b16 only: 192 bytes = 48 dwords, the 96 columns and no pad.  A 32-lane half reads 4 rows (q4) x 16 dwords;
//     48 q4 mod 64 = 0, 48, 32, 16 gives each row a quarter of the banks of its own: conflict-free.  (A shared pitch of 4 x odd dwords, such as
//     the 36 of the head_dim-64 tiles or 52 here, leaves two of the four rows overlapping on some banks.)
// ---------------------------------------------------------------------------------------------------------------------
constexpr int MA_HD = 80;
constexpr int MA_KP = 176;                     // bytes per staged K row
constexpr int MA_VP = 192;                     // bytes per staged V row: 96 bf16
constexpr int MA_CHUNKS = AT_KT * (MA_HD / 8); // 16-byte chunks of one staged tile: 640 for 256 threads

struct MaArgs {
  const unsigned short* qkv;       // [B][T][3C] bf16
  unsigned short* ctx;             // [B][T][C] bf16
  const int* key_len;
  int t, c;
  float scale_log2e;
};

// K and V rows k0 .. k0 + 63 of one (clip, head) into LDS, 10 chunks of 16 bytes per row (rows past t clamped to t - 1: their probabilities are 0)
__device__ __forceinline__ void ma_stage_kv(char* ks_, char* vs_, const unsigned short* base, size_t rowp, int c, int t, int k0, int tid) {
#pragma unroll
  for (int rep = 0; rep < 3; ++rep) {
    const int chunk = tid + 256 * rep;
    if (chunk < MA_CHUNKS) {
      const int r = chunk / 10, cc = chunk - 10 * r;
      const int key = k0 + r < t ? k0 + r : t - 1;
      const unsigned short* src = base + (size_t)key * rowp + cc * 8;
      *reinterpret_cast<uint4*>(ks_ + r * MA_KP + cc * 16) = *reinterpret_cast<const uint4*>(src + c);
      *reinterpret_cast<uint4*>(vs_ + r * MA_VP + cc * 16) = *reinterpret_cast<const uint4*>(src + 2 * c);
    }
  }
}

// S^T = K Q^T of 32-key sub-tile `sub`; accumulator register i <-> key k0 + 32 sub + 16 (i / 8) + 8 half + i % 8 (the order mask_tail expects)
__device__ __forceinline__ f32x16 ma_qk_subtile(const char* ks_, int sub, const TileLane& g, const s16x8 (&qf)[5]) {
  f32x16 s;
  zero(s);
  const char* kr = ks_ + (sub * 32 + g.pm) * MA_KP + g.half * 16;
#pragma unroll
  for (int ks = 0; ks < 5; ++ks) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const s16x8*>(kr + ks * 32), qf[ks], s, 0, 0, 0);
  return s;
}

// two ds_read_b64_tr_b16 out of the V tile: the 8 A-operand elements of one k-step of 16 keys
__device__ __forceinline__ s16x8 ma_tr8(const char* p) {
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((TS_LDS s16x4*)((TS_LDS char*)p));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((TS_LDS s16x4*)((TS_LDS char*)p + 4 * MA_VP));
  return s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// o^T[d][query] += V^T P^T over the 32 keys of sub-tile `sub`; o[mt] holds d = 32 mt .. 32 mt + 31 (d >= 80: the zeroed pad columns)
__device__ __forceinline__ void ma_acc_pv(f32x16 (&o)[3], const f32x16& p, const char* vs_, int sub, int tr_off) {
#pragma unroll
  for (int ks2 = 0; ks2 < 2; ++ks2) {
    const unsigned p01 = pack_bf16(p[8 * ks2 + 0], p[8 * ks2 + 1]), p23 = pack_bf16(p[8 * ks2 + 2], p[8 * ks2 + 3]);
    const unsigned p45 = pack_bf16(p[8 * ks2 + 4], p[8 * ks2 + 5]), p67 = pack_bf16(p[8 * ks2 + 6], p[8 * ks2 + 7]);
    const s16x8 pb = __builtin_bit_cast(s16x8, uint4{p01, p23, p45, p67});
#pragma unroll
    for (int mt = 0; mt < 3; ++mt)
      o[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ma_tr8(vs_ + (sub * 32 + 16 * ks2) * MA_VP + tr_off + 64 * mt), pb, o[mt], 0, 0, 0);
  }
}

// amdgpu_waves_per_eu(4, 4), as w2v_flash_attn_kernel: the loop is bound by the softmax's quarter-rate exp2, which only other resident waves hide.
// The compiler reports 128 VGPRs (48 accumulators, 20 of Q, 16 of scores, the K / V fragments in flight), occupancy 4, 23552 bytes of LDS, and
// 3 spilled VGPRs (16 bytes of scratch); in the generated code the scratch stores sit before the key loop and the reloads after it.  The
// budget of 4 waves forces that spill; (3, 3), which would have none, has not been timed against it.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void mms_flash_attn_kernel(const MaArgs a) {
  __shared__ __attribute__((aligned(16))) char ks_[AT_KT * MA_KP];
  __shared__ __attribute__((aligned(16))) char vs_[AT_KT * MA_VP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, head = blockIdx.y;
  const int q0 = blockIdx.x * AT_QW + wave * 32;
  const size_t rowp = (size_t)3 * a.c;
  const unsigned short* base = a.qkv + (size_t)b * a.t * rowp + (size_t)head * MA_HD;
  const int lim = key_limit<true>(a.key_len, b, a.t);
  const TileLane g = tile_lane(lane);
  const int tr_off = (8 * g.half + ((lane >> 2) & 3)) * MA_VP + (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;   // tile_lane's, at this tile's pitch
  const int query = q0 + g.n32;
  // the pad columns 80 .. 95 of the 64 staged V rows, once (two 16-byte chunks per row); the loop's first barrier orders it before any read
  if (tid < 128) *reinterpret_cast<uint4*>(vs_ + (tid >> 1) * MA_VP + (10 + (tid & 1)) * 16) = uint4{0u, 0u, 0u, 0u};
  s16x8 qf[5];
  {
    const uint4* p4 = reinterpret_cast<const uint4*>(base + (size_t)(query < a.t ? query : a.t - 1) * rowp + 8 * g.half);
#pragma unroll
    for (int ks = 0; ks < 5; ++ks) qf[ks] = __builtin_bit_cast(s16x8, p4[2 * ks]);
  }
  f32x16 o[3];
  zero(o[0]); zero(o[1]); zero(o[2]);
  float m_run = -INFINITY, l_run = 0.f;

  for (int k0 = 0; k0 < lim; k0 += AT_KT) {
    __syncthreads();                                                          // the previous tile has been consumed
    ma_stage_kv(ks_, vs_, base, rowp, a.c, a.t, k0, tid);
    __syncthreads();
    const bool full = k0 + AT_KT <= lim;                                      // no masked key in this tile (uniform)
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      if (k0 + sub * 32 >= lim) break;                                        // uniform: nothing but masked keys
      f32x16 s = ma_qk_subtile(ks_, sub, g, qf);
      if (!full) s = mask_tail(s, k0 + sub * 32 + 8 * g.half, lim);
      const SoftmaxStep sm = softmax_step<true>(s, m_run, l_run, a.scale_log2e);
      m_run = sm.m; l_run = sm.l;
      if (__any(sm.alpha != 1.f)) {                                           // after the first tiles the running maximum rarely moves
#pragma unroll
        for (int mt = 0; mt < 3; ++mt)
#pragma unroll
          for (int i = 0; i < 16; ++i) o[mt][i] *= sm.alpha;
      }
      ma_acc_pv(o, sm.p, vs_, sub, tr_off);
    }
  }
  const float l = l_run + __shfl_xor(l_run, 32);
  const float inv = 1.f / l;
  if (query < a.t) {
    // accumulator registers 4 gg .. 4 gg + 3 of block mt <-> d = 32 mt + 8 gg + 4 half + 0..3; the third block stops at d = 80
    unsigned short* dst = a.ctx + ((size_t)b * a.t + query) * a.c + (size_t)head * MA_HD + 4 * g.half;
#pragma unroll
    for (int mt = 0; mt < 3; ++mt)
#pragma unroll
      for (int gg = 0; gg < (mt < 2 ? 4 : 2); ++gg)
        *reinterpret_cast<uint2*>(dst + 32 * mt + 8 * gg) =
            uint2{pack_bf16(o[mt][4 * gg] * inv, o[mt][4 * gg + 1] * inv), pack_bf16(o[mt][4 * gg + 2] * inv, o[mt][4 * gg + 3] * inv)};
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The attention adapter with the LayerNorm behind it.  The tile layout, the two matrix-core products and the LayerNorm statistics are
// csrc/mms_adapter_rows.hpp's (shared with the adapter's backward, csrc/mms_adapter_train.hip).
// Every weight is read once per workgroup (from L2) for its 16 rows: 2 a c / 16 values per row next to the row's own 2 c.
// p.in: the rows are read from there and written to p.h (the training forward, which keeps its input); NULL: in place on p.h.
// ---------------------------------------------------------------------------------------------------------------------
template <int NQ, int NW, bool BF>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(AD_WAVES, AD_WAVES))) void mms_adapter_kernel(const AdArgs p) {
  __shared__ float red[4][NW * 16];
  __shared__ __attribute__((aligned(16))) float zp[NW][16][AD_ZP];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // scalar: the tests on the wave's columns below are uniform branches
  const int rl = lane & 15, g = lane >> 4;
  const long long row = (long long)blockIdx.x * 16 + rl;
  const bool row_ok = row < p.rows;
  const long long row_off = (row_ok ? row : p.rows - 1) * p.c;  // rows past the end: the last row again, never stored
  float* hr = p.h + row_off;
  const int c = p.c, a = p.a;
  const int col0 = 16 * wave * NQ + 4 * g;                      // the lane's columns of chunk i: col0 + 16 i + 0..3
  f32x4 v[NQ];
  float mu, rs;
  ad_load_stats<NQ, NW>(p.in ? p.in + row_off : hr, c, col0, v, red[0], red[1], wave, rl, g, mu, rs);

  // ---- z = LN(h) W1^T: this wave's columns; the partial tile goes to zp[wave][row][j]
  ad_prod_in<NQ, NW, BF, false>([&](int i) { return ad_xhat(v[i], col0 + 16 * i, c, mu, rs, p.norm_w, p.norm_b); }, p.w1, c, a, wave, rl, g, col0, zp);
  __syncthreads();
  // relu(z + b1)[row][j], summed over the waves in a fixed order
  auto zval = [&](int j) -> float {
    if (j >= a) return 0.f;
    return fmaxf(ad_zsum<NW>(zp, p.b1[j], rl, j), 0.f);
  };

  // ---- h^T += W2 relu(z)^T, chunk by chunk; then + b2
  if constexpr (BF) {
    s16x8 zb[2];
    ad_out_b(zval, g, zb);
    const unsigned short* w2 = static_cast<const unsigned short*>(p.w2);
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const int cm = 16 * (wave * NQ + i) + rl;                  // A operand: this lane's W2 row (= output column)
      if (cm - rl >= c) break;                                   // uniform
      v[i] = ad_out_chunk<false>(v[i], w2, cm, c, a, g, zb);
      if (i % 4 == 3 && i + 1 < NQ) AD_FENCE;
    }
  } else {
    float zf[16];
    ad_out_b(zval, g, zf);
    const float* w2 = static_cast<const float*>(p.w2);
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const int cm = 16 * (wave * NQ + i) + rl;
      if (cm - rl >= c) break;
      v[i] = ad_out_chunk<false>(v[i], w2, cm, c, a, g, zf);
      if (i % 4 == 3 && i + 1 < NQ) AD_FENCE;
    }
  }
  AD_MFMA_DRAIN;                                                 // as above, before the tile's accumulators are read by vector instructions
  float s2 = 0.f;
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    const int col = col0 + 16 * i;
    if (col < c) {
      v[i] += *reinterpret_cast<const f32x4*>(p.b2 + col);
      if (row_ok) *reinterpret_cast<f32x4*>(hr + col) = v[i];
      s2 += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    }
    if (i % 4 == 3) AD_FENCE;
  }
  if (!p.next_w) return;                                         // uniform

  // ---- the LayerNorm that follows, on the updated row
  const float mu2 = ad_row_sum<NW>(s2, red[2], wave, rl, g) / c;
  float q2 = 0.f;
#pragma unroll
  for (int i = 0; i < NQ; ++i)
    if (col0 + 16 * i < c) {
      const f32x4 d = v[i] - mu2;
      q2 += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
    }
  const float rs2 = rsqrtf(ad_row_sum<NW>(q2, red[3], wave, rl, g) / c + p.next_eps);
  if (!row_ok) return;
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    const int col = col0 + 16 * i;
    if (col < c) {
      const f32x4 w4 = *reinterpret_cast<const f32x4*>(p.next_w + col), b4 = *reinterpret_cast<const f32x4*>(p.next_b + col);
      const f32x4 y = (v[i] - mu2) * rs2 * w4 + b4;
      if (p.y_next) *reinterpret_cast<f32x4*>(p.y_next + row * c + col) = y;
      if (p.y_next16) *reinterpret_cast<uint2*>(p.y_next16 + row * c + col) = uint2{pack_bf16(y[0], y[1]), pack_bf16(y[2], y[3])};
    }
    if (i % 4 == 3) AD_FENCE;
  }
}

}  // namespace ts

using namespace ts;

extern "C" int ts_mms_abi_version(void) { return TS_MMS_ABI_VERSION; }

extern "C" int ts_mms_attention_fwd(const void* qkv, int32_t batch, int32_t t, int32_t c, int32_t heads, const int32_t* key_len, void* ctx,
                                    void* stream_) {
  if (!qkv || !ctx || batch <= 0 || t <= 0 || c <= 0 || heads <= 0 || c % heads) return TS_EINVAL;
  if (c / heads != MA_HD || misaligned(qkv) || misaligned(ctx) || heads > 65535 || batch > 65535) return TS_EUNSUPPORTED;
  TS_STREAM;
  MaArgs f{};
  f.qkv = static_cast<const unsigned short*>(qkv); f.ctx = static_cast<unsigned short*>(ctx); f.key_len = key_len;
  f.t = t; f.c = c; f.scale_log2e = LOG2E / sqrtf((float)MA_HD);
  hipLaunchKernelGGL(mms_flash_attn_kernel, dim3((t + AT_QW - 1) / AT_QW, heads, batch), dim3(256), 0, stream, f);
  return hip_status(hipGetLastError());
}

int ts::adapter_launch(const AdArgs& p, int precision, hipStream_t stream) {
  const int c = p.c;
  const dim3 grid((unsigned)((p.rows + 15) / 16));
#define TS_AD(NQ_, NW_)                                                                                              \
  do {                                                                                                               \
    if (precision) hipLaunchKernelGGL((mms_adapter_kernel<NQ_, NW_, true>), grid, dim3(NW_ * 64), 0, stream, p);     \
    else hipLaunchKernelGGL((mms_adapter_kernel<NQ_, NW_, false>), grid, dim3(NW_ * 64), 0, stream, p);              \
  } while (0)
  // NW waves x NQ chunks of 16 columns cover c.  At most 10 chunks per wave up to c = 2048: 72 .. 122 VGPRs, no scratch, occupancy 4 (compiler's
  // report); wider rows (no published checkpoint has them) take 16 chunks on 16 waves, where the 128-VGPR budget of 1024 threads makes the
  // compiler spill: 93 VGPRs (184 bytes of scratch) in the bf16 kernel, 388 (180 bytes) in the f32 one
  if (c <= 256) TS_AD(4, 4);
  else if (c <= 512) TS_AD(8, 4);
  else if (c <= 1024) TS_AD(8, 8);
  else if (c <= 1280) TS_AD(10, 8);
  else if (c <= 2048) TS_AD(8, 16);
  else TS_AD(16, 16);
#undef TS_AD
  return hip_status(hipGetLastError());
}

extern "C" int ts_mms_attn_adapter_fwd(float* h, int64_t rows, int32_t c, int32_t a, const float* norm_w, const float* norm_b, const void* w1,
                                       const float* b1, const void* w2, const float* b2, const float* next_w, const float* next_b, float next_eps,
                                       float* y_next, void* y_next_op, int32_t precision, void* stream_) {
  if (!h || !norm_w || !norm_b || !w1 || !b1 || !w2 || !b2 || rows <= 0 || c <= 0 || a <= 0) return TS_EINVAL;
  if (next_w && (!next_b || (!y_next && !y_next_op))) return TS_EINVAL;
  if (a % 16 || a > 64 || c % 8 || c > 4096 || precision < 0 || precision > 1 || (y_next_op && !precision)) return TS_EUNSUPPORTED;
  if (misaligned(h) || misaligned(norm_w) || misaligned(norm_b) || misaligned(w1) || misaligned(b1) || misaligned(w2) || misaligned(b2) ||
      misaligned(next_w) || misaligned(next_b) || misaligned(y_next) || misaligned(y_next_op, 7))
    return TS_EUNSUPPORTED;
  if ((rows + 15) / 16 > 0x7fffffffLL) return TS_EUNSUPPORTED;
  TS_STREAM;
  AdArgs p{};
  p.h = h; p.rows = rows; p.c = c; p.a = a; p.norm_w = norm_w; p.norm_b = norm_b; p.b1 = b1; p.b2 = b2; p.w1 = w1; p.w2 = w2;
  p.next_w = next_w; p.next_b = next_b; p.next_eps = next_eps;
  p.y_next = next_w ? y_next : nullptr; p.y_next16 = next_w ? static_cast<unsigned short*>(y_next_op) : nullptr;
  return adapter_launch(p, precision, stream);
}
