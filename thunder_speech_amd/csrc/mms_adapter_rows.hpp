// The row code of the MMS attention adapter, shared by its inference / training forward (mms_adapter_kernel, csrc/mms.hip), the language bank's
// forward (mms_lang_adapter_kernel, csrc/mms_lang_bank.hip) and its backward (csrc/mms_adapter_train.hip).  Workgroup = 16 rows, NW waves; the row tile lives in registers, split by columns: the columns come in chunks of
// 16, wave w owns chunks w NQ .. w NQ + NQ - 1, and lane (row = lane & 15, g = lane >> 4) holds columns 16 q + 4 g .. + 3 of its row for each of
// them (one f32x4 per chunk).  That is the accumulator layout of a 16 x 16 MFMA whose N index is the row and whose M index is the column, so both
// kinds of product run on the matrix cores without moving the tile:
//   "in"   z[row][j]   = sum_col x[row][col] W[j][col]     A = x (M = row), B = W (N = j), contraction over the lane's own columns -- the order of
//                                                          a contraction is free, so a k-step is simply the next 32 (bf16) / 4 (f32) columns the
//                                                          lanes hold; every wave sums its own columns, the NW partial sums meet in LDS
//   "out"  t^T[col][row] += sum_j W[col][j] z[row][j]      A = W (M = col), B = z^T (N = row), C = a chunk of the tile
// The forward multiplies by W1 [a][c] going in and W2 [c][a] going out.  The backward runs the same two products with the other matrix each
// (dy W2 going in, W1^T dz going out): TR = true reads the weight through its transpose, element by element (k runs along the matrix's rows).
// precision 1: v_mfma_f32_16x16x32_bf16 (a = 16 fills half a k-step: the other half is zeros); precision 0: v_mfma_f32_16x16x4_f32.
#pragma once
#include "ts_common.hpp"

namespace ts {

struct AdArgs {
  const float* in;               // rows are read from here; NULL = from h (in place)
  float* h;                      // rows are written here
  long long rows;
  int c, a;
  const float *norm_w, *norm_b, *b1, *b2, *next_w, *next_b;
  const void *w1, *w2;
  float next_eps;
  float* y_next;
  unsigned short* y_next16;
};
// launches mms_adapter_kernel for checked arguments (csrc/mms.hip)
int adapter_launch(const AdArgs& p, int precision, hipStream_t stream);

// The argument checks of ts_mms_attn_adapter_fwd (thunder_speech_amd/mms.h) that do not concern the number of rows: 0, TS_EINVAL or TS_EUNSUPPORTED
inline int ad_check_args(const float* h, int c, int a, const float* norm_w, const float* norm_b, const void* w1, const float* b1, const void* w2,
                         const float* b2, const float* next_w, const float* next_b, const float* y_next, const void* y_next_op, int precision) {
  if (!h || !norm_w || !norm_b || !w1 || !b1 || !w2 || !b2 || c <= 0 || a <= 0) return TS_EINVAL;
  if (next_w && (!next_b || (!y_next && !y_next_op))) return TS_EINVAL;
  if (a % 16 || a > 64 || c % 8 || c > 4096 || precision < 0 || precision > 1 || (y_next_op && !precision)) return TS_EUNSUPPORTED;
  if (misaligned(h) || misaligned(norm_w) || misaligned(norm_b) || misaligned(w1) || misaligned(b1) || misaligned(w2) || misaligned(b2) ||
      misaligned(next_w) || misaligned(next_b) || misaligned(y_next) || misaligned(y_next_op, 7))
    return TS_EUNSUPPORTED;
  return TS_OK;
}

// The one place that maps c to a tile shape: f(NQ, NW) as integral constants.  NW waves x NQ chunks of 16 columns cover c.  At most 10 chunks
// per wave up to c = 2048: 72 .. 122 VGPRs, no scratch, occupancy 4 (compiler's report); wider rows (no published checkpoint has them) take 16
// chunks on 16 waves, where the 128-VGPR budget of 1024 threads makes the compiler spill: 93 VGPRs (184 bytes of scratch) in the bf16 kernel,
// 388 (180 bytes) in the f32 one.  The shape fixes the order of every sum of a row, so launchers that must agree bit for bit share it.
template <int V>
struct AdInt { static constexpr int value = V; };
template <class F>
inline void ad_tile_shape(int c, F&& f) {
  if (c <= 256) f(AdInt<4>{}, AdInt<4>{});
  else if (c <= 512) f(AdInt<8>{}, AdInt<4>{});
  else if (c <= 1024) f(AdInt<8>{}, AdInt<8>{});
  else if (c <= 1280) f(AdInt<10>{}, AdInt<8>{});
  else if (c <= 2048) f(AdInt<8>{}, AdInt<16>{});
  else f(AdInt<16>{}, AdInt<16>{});
}

constexpr int AD_WAVES = 4;    // waves per SIMD the register budget is set for: the launch is bound by memory, the resident workgroups overlap their phases
// The chunk loops are fully unrolled (the tile is a register array) and the scheduler would hoist every chunk's weight loads to the top: twice the
// tile in registers.  A scheduling fence every 4 chunks keeps 4 chunks' loads in flight and the rest of the budget for the tile.
#define AD_FENCE __builtin_amdgcn_sched_barrier(0)
// 16 wait states: more than the 11 an 8-pass MFMA's result needs before a vector / LDS / memory instruction may read it
#define AD_MFMA_DRAIN                               \
  do {                                              \
    __builtin_amdgcn_sched_barrier(0);              \
    asm volatile("s_nop 15" ::: "memory");          \
    __builtin_amdgcn_sched_barrier(0);              \
  } while (0)
constexpr int AD_ZP = 68;      // floats per row of a wave's partial z tile (64 + 4)

// sum of `v` over the whole row (all columns, all waves), in every lane of the row; red = [NW][16] floats of its own per call
template <int NW>
__device__ __forceinline__ float ad_row_sum(float v, float* red, int wave, int rl, int g) {
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  if (g == 0) red[wave * 16 + rl] = v;
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int w = 0; w < NW; ++w) s += red[w * 16 + rl];
  return s;
}

// the lane's part of row hr into v (0 outside the row), and the row's LayerNorm statistics (mean, then the centred sum of squares, as
// w2v_layernorm_kernel; eps 1e-5): lane -> row's 4 lanes -> the NW waves through LDS.  red0 / red1: [NW][16] floats each.
template <int NQ, int NW>
__device__ __forceinline__ void ad_load_stats(const float* hr, int c, int col0, f32x4 (&v)[NQ], float* red0, float* red1, int wave, int rl, int g,
                                              float& mu, float& rs) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    const int col = col0 + 16 * i;
    v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (col < c) v[i] = *reinterpret_cast<const f32x4*>(hr + col);
    s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
  }
  mu = ad_row_sum<NW>(s, red0, wave, rl, g) / c;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < NQ; ++i)
    if (col0 + 16 * i < c) {
      const f32x4 d = v[i] - mu;
      q += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
    }
  rs = rsqrtf(ad_row_sum<NW>(q, red1, wave, rl, g) / c + 1e-5f);
}

// LN(h) of the chunk at column `col`, 0 outside the row
__device__ __forceinline__ f32x4 ad_xhat(const f32x4& vi, int col, int c, float mu, float rs, const float* norm_w, const float* norm_b) {
  if (col >= c) return f32x4{0.f, 0.f, 0.f, 0.f};
  const f32x4 w4 = *reinterpret_cast<const f32x4*>(norm_w + col), b4 = *reinterpret_cast<const f32x4*>(norm_b + col);
  return (vi - mu) * rs * w4 + b4;
}

// four / eight bf16 elements `stride` apart, packed in order (the transposed reads of TR = true)
__device__ __forceinline__ uint2 ad_gather4(const unsigned short* p, size_t stride) {
  return uint2{(unsigned)p[0] | ((unsigned)p[stride] << 16), (unsigned)p[2 * stride] | ((unsigned)p[3 * stride] << 16)};
}
__device__ __forceinline__ uint4 ad_gather8(const unsigned short* p, size_t stride) {
  const uint2 lo = ad_gather4(p, stride), hi = ad_gather4(p + 4 * stride, stride);
  return uint4{lo.x, lo.y, hi.x, hi.y};
}

// ---- the "in" product: zp[wave][row][j] = sum over this wave's columns of x[row][col] W[j][col], 16 outputs j at a time.  x(i) = the lane's f32x4 of
// chunk i (0 outside the row).  W: [a][c] (TR = false) or [c][a] read as its transpose (TR = true).  The caller's __syncthreads() follows.
template <int NQ, int NW, bool BF, bool TR, class X>
__device__ __forceinline__ void ad_prod_in(X&& x, const void* w, int c, int a, int wave, int rl, int g, int col0, float (*zp)[16][AD_ZP]) {
  for (int na = 0; na < a / 16; ++na) {
    const int j = 16 * na + rl;                                  // B operand: this lane's W row
    f32x4 z = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (BF) {
      const unsigned short* w1r = static_cast<const unsigned short*>(w) + (TR ? (size_t)j : (size_t)j * c);
#pragma unroll
      for (int i = 0; i < NQ; i += 2) {
        if (16 * (wave * NQ + i) >= c) break;                    // uniform: the wave's columns end here
        const f32x4 x0 = x(i), x1 = x(i + 1);
        const s16x8 af = __builtin_bit_cast(s16x8, uint4{pack_bf16(x0[0], x0[1]), pack_bf16(x0[2], x0[3]), pack_bf16(x1[0], x1[1]), pack_bf16(x1[2], x1[3])});
        const int ca = col0 + 16 * i, cb = ca + 16;
        uint2 wa = uint2{0u, 0u}, wb = uint2{0u, 0u};
        if constexpr (TR) {
          if (ca < c) wa = ad_gather4(w1r + (size_t)ca * a, a);
          if (cb < c) wb = ad_gather4(w1r + (size_t)cb * a, a);
        } else {
          if (ca < c) wa = *reinterpret_cast<const uint2*>(w1r + ca);
          if (cb < c) wb = *reinterpret_cast<const uint2*>(w1r + cb);
        }
        z = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, __builtin_bit_cast(s16x8, uint4{wa.x, wa.y, wb.x, wb.y}), z, 0, 0, 0);
        if (i % 4 == 2 && i + 2 < NQ) AD_FENCE;
      }
    } else {
      const float* w1r = static_cast<const float*>(w) + (TR ? (size_t)j : (size_t)j * c);
#pragma unroll
      for (int i = 0; i < NQ; ++i) {
        if (16 * (wave * NQ + i) >= c) break;
        const f32x4 x0 = x(i);
        const int ca = col0 + 16 * i;
        f32x4 w4 = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (TR) {
          if (ca < c) w4 = f32x4{w1r[(size_t)ca * a], w1r[(size_t)(ca + 1) * a], w1r[(size_t)(ca + 2) * a], w1r[(size_t)(ca + 3) * a]};
        } else {
          if (ca < c) w4 = *reinterpret_cast<const f32x4*>(w1r + ca);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) z = __builtin_amdgcn_mfma_f32_16x16x4f32(x0[r], w4[r], z, 0, 0, 0);
        if (i % 4 == 3 && i + 1 < NQ) AD_FENCE;
      }
    }
    // The last MFMA of the chain must have retired before the LDS store reads its result.  Measured without this wait: exactly the last
    // k-step's contribution was missing from z (one-hot weights, c = 160) -- the compiler had put no wait states between that MFMA and the store.
    // Seen with hipcc of ROCm 7.2.0 (HIP 7.2.26015, AMD clang 22.0.0git roc-7.2.0): the MFMA ends one basic block, the store opens the next.
    AD_MFMA_DRAIN;
    // accumulator register r of lane (n = rl, g): row 4 g + r, output j = 16 na + rl
#pragma unroll
    for (int r = 0; r < 4; ++r) zp[wave][4 * g + r][16 * na + rl] = z[r];
  }
}

// bias + the NW partial sums of zp[.][row][j], in a fixed order (bias = 0 where there is none)
template <int NW>
__device__ __forceinline__ float ad_zsum(const float (*zp)[16][AD_ZP], float bias, int row, int j) {
  float t = bias;
#pragma unroll
  for (int w = 0; w < NW; ++w) t += zp[w][row][j];
  return t;
}

// ---- the "out" product.  B operands of a lane's row from zval(j) (0 for j >= a):
//   bf16: k-step ks holds j = 32 ks + 8 g + 0..7;   f32: k-step sidx holds j = 4 sidx + g
template <class Z>
__device__ __forceinline__ void ad_out_b(Z&& zval, int g, s16x8 (&zb)[2]) {
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    float e[8];
#pragma unroll
    for (int x = 0; x < 8; ++x) e[x] = zval(32 * ks + 8 * g + x);
    zb[ks] = __builtin_bit_cast(s16x8, uint4{pack_bf16(e[0], e[1]), pack_bf16(e[2], e[3]), pack_bf16(e[4], e[5]), pack_bf16(e[6], e[7])});
  }
}
template <class Z>
__device__ __forceinline__ void ad_out_b(Z&& zval, int g, float (&zf)[16]) {
#pragma unroll
  for (int sidx = 0; sidx < 16; ++sidx) zf[sidx] = zval(4 * sidx + g);
}
// acc (columns 16 q + 4 g + 0..3 of row rl) += W[cm][.] z, cm = 16 q + rl this lane's A row (= output column).  W: [c][a], or [a][c] read as
// its transpose (TR)
template <bool TR>
__device__ __forceinline__ f32x4 ad_out_chunk(f32x4 acc, const unsigned short* w, int cm, int c, int a, int g, const s16x8 (&zb)[2]) {
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    if (32 * ks >= a) break;
    const int j = 32 * ks + 8 * g;
    uint4 wf = uint4{0u, 0u, 0u, 0u};
    if (cm < c && j < a) {
      if constexpr (TR) wf = ad_gather8(w + (size_t)j * c + cm, c);
      else wf = *reinterpret_cast<const uint4*>(w + (size_t)cm * a + j);
    }
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(s16x8, wf), zb[ks], acc, 0, 0, 0);
  }
  return acc;
}
template <bool TR>
__device__ __forceinline__ f32x4 ad_out_chunk(f32x4 acc, const float* w, int cm, int c, int a, int g, const float (&zf)[16]) {
  const int cc = cm < c ? cm : c - 1;
  const float* w2r = TR ? w + (size_t)g * c + cc : w + (size_t)cc * a + g;
  const size_t step = TR ? (size_t)4 * c : (size_t)4;
#pragma unroll
  for (int sidx = 0; sidx < 16; ++sidx) {
    if (4 * sidx >= a) break;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(cm < c ? w2r[sidx * step] : 0.f, zf[sidx], acc, 0, 0, 0);
  }
  return acc;
}

// ---- the adapter's forward on one workgroup's 16 rows, with the LayerNorm behind it: the body of mms_adapter_kernel (csrc/mms.hip) and of the
// language bank's kernel (csrc/mms_lang_bank.hip), which differ in where a tile's rows and tensors lie.  `row`: the lane's row of p.h / p.in /
// p.y_next; !row_ok: a row past the end, which repeats a valid one and is never stored.  Every weight is read once per workgroup (from L2) for
// its 16 rows: 2 a c / 16 values per row next to the row's own 2 c.
template <int NQ, int NW, bool BF>
__device__ __forceinline__ void ad_fwd_tile(const AdArgs& p, long long row, bool row_ok) {
  __shared__ float red[4][NW * 16];
  __shared__ __attribute__((aligned(16))) float zp[NW][16][AD_ZP];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // scalar: the tests on the wave's columns below are uniform branches
  const int rl = lane & 15, g = lane >> 4;
  const long long row_off = row * p.c;
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
      if (p.y_next) *reinterpret_cast<f32x4*>(p.y_next + row_off + col) = y;
      if (p.y_next16) *reinterpret_cast<uint2*>(p.y_next16 + row_off + col) = uint2{pack_bf16(y[0], y[1]), pack_bf16(y[2], y[3])};
    }
    if (i % 4 == 3) AD_FENCE;
  }
}

}  // namespace ts
