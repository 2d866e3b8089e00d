// MXFP8 inference of the wav2vec2 encoder layers on the block-scaled matrix-core instruction of gfx950 (include_staged/thunder_speech_amd/mxfp8.h):
//   ts_mx_quantize_rows   bf16 / f32 rows -> MX operand (e4m3fn elements + one e8m0 scale byte per 32 consecutive K elements)
//   ts_mx_layernorm_fwd   the LayerNorm row of w2v_layernorm_kernel (csrc/w2v_rows.hip), written as an MX operand (and f32 on request)
//   ts_mx_pack_w          a quantised weight permuted into the fragment order the product loads
//   ts_mx_gemm_nt         y = act(x w^T + bias) (+ y) over MX operands on v_mfma_scale_f32_16x16x128_f8f6f4 (cbsz = blgp = 0: e4m3 x e4m3)
//
// The quantiser is one function (mx_scale_byte / mx_pack4) for every writer of an MX operand; the rule is the header's.
//
// Operand map of v_mfma_scale_f32_16x16x128_f8f6f4 as this file uses it (tests/test_gpu_mxfp8_kernels.py checks it with exact integer data):
// lane l (r = l & 15, g = l >> 4) holds row r (A) / column r (B); its operand registers 0-3 hold K = 16 g .. 16 g + 15 of the 128-deep step and
// registers 4-7 hold K = 64 + 16 g .. 64 + 16 g + 15.  The scale operand's byte 0 (opsel 0) of lane l scales row / column r over the 32-deep
// block g, K = 32 g .. 32 g + 31 -- which lanes 2 (g & 1) and 2 (g & 1) + 1 of the row hold, in their lower (g < 2) or upper registers -- by
// 2^(byte - 127).  C / D: column l & 15, rows 4 (l >> 4) + reg.
//
// The product: 128 x 128 output tile per workgroup, 4 waves as 2 x 2, a wave owns 64 x 64 = 4 x 4 accumulator blocks.  Per 128-deep step the
// A tile (128 rows x 128 bytes) and its scale dwords pass through a double-buffered LDS image (registers -> ds_write_b128, 16-byte chunks
// XOR-swizzled by row so that the fragment reads cover all banks); the B fragments and their scales are static, packed once by ts_mx_pack_w in
// lane order, and go from L2 straight into registers, each column block re-requested for the next step right behind its last MFMA of this one.
// Every wait is the compiler's.
// Epilogue: each wave stages 64 rows x 32 columns of f32 in its own 8 KiB of the idle operand image and leaves row-wise -- 16 bytes per lane of
// f32, 8 of bf16, 4 of e4m3; a quantisation block of the GELU -> MX epilogue is the 8 lanes of one row segment.
#include "w2v_rows.hpp"

#include "thunder_speech_amd/mxfp8.h"

namespace ts {

namespace {

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef unsigned char u8;

constexpr int MXM = TS_MX_GEMM_TILE_ROWS, MXN = TS_MX_GEMM_TILE_COLS, MXK = 128;
constexpr int MX_ABYTES = MXM * MXK;             // 16 KiB: the A tile of one step
constexpr int MX_SBYTES = MXM * 4;               // its scale dwords
constexpr int MX_LDS = 2 * MX_ABYTES + 2 * MX_SBYTES;

// ---- the quantiser ----------------------------------------------------------------------------------------------------
// scale byte e + 127 of a block with amax >= 0 (finite): e = floor(log2 amax) - 8 from the exponent field, + 1 when the mantissa is above 1.75
// (amax 2^-e > 448), clamped below at -127 (f32 cannot reach the upper clamp: e <= 120).  amax == 0 gives 0.
__device__ __forceinline__ unsigned mx_scale_byte(float amax) {
  const unsigned u = __float_as_uint(amax);
  int e = (int)(u >> 23) - 135 + ((u & 0x7fffffu) > 0x600000u ? 1 : 0);
  e = e < -127 ? -127 : (e > 127 ? 127 : e);
  return (unsigned)(e + 127);
}
// 2^-e as a float: always normal, exponent field 254 - byte in [7, 254]
__device__ __forceinline__ float mx_multiplier(unsigned byte) { return __uint_as_float((254u - byte) << 23); }
// four values of a block -> four e4m3fn bytes (v_cvt_pk_fp8_f32: OCP on gfx950, round-to-nearest-even, subnormals kept); a zero block -> 0
__device__ __forceinline__ unsigned mx_pack4(float a, float b, float c, float d, float mult, bool zero_block) {
  int p = __builtin_amdgcn_cvt_pk_fp8_f32(a * mult, b * mult, 0, false);
  p = __builtin_amdgcn_cvt_pk_fp8_f32(c * mult, d * mult, p, true);
  return zero_block ? 0u : (unsigned)p;
}
__device__ __forceinline__ float amax4(float a, float b, float c, float d) { return fmaxf(fmaxf(fabsf(a), fabsf(b)), fmaxf(fabsf(c), fabsf(d))); }
// maximum over aligned groups of LANES (4 or 8) consecutive lanes, every lane of a group active: two quad permutes (lane ^ 1, lane ^ 2) and, for 8,
// the mirror of the row's half (lane -> 7 - lane: the other quad, whose four lanes already agree) -- DPP moves, no LDS round trip
template <int CTRL>
__device__ __forceinline__ float dpp_max(float v) {
  return fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true)));
}
template <int LANES>
__device__ __forceinline__ float group_max(float v) {
  static_assert(LANES == 4 || LANES == 8, "a block is 4 or 8 lanes");
  v = dpp_max<0xB1>(v);                          // quad_perm [1, 0, 3, 2]
  v = dpp_max<0x4E>(v);                          // quad_perm [2, 3, 0, 1]
  if (LANES == 8) v = dpp_max<0x141>(v);         // row_half_mirror
  return v;
}

// ---- ts_mx_quantize_rows: one thread per 8 elements, a block is 4 consecutive lanes ---------------------------------------
template <bool BF>
__global__ __launch_bounds__(256) void mx_quantize_kernel(const void* __restrict__ src, long long ld, long long rows, int k, u8* __restrict__ q,
                                                          long long ldq, u8* __restrict__ sc, long long lds) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const int per = k >> 3;
  const bool valid = idx < rows * per;           // k % 32 == 0: the 4 lanes of a block are valid together
  const long long row = valid ? idx / per : 0;
  const int col = valid ? (int)(idx - row * per) * 8 : 0;
  float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (valid) {
    if (BF) {
      const u32x4 p = *reinterpret_cast<const u32x4*>(static_cast<const unsigned short*>(src) + row * ld + col);
#pragma unroll
      for (int i = 0; i < 4; ++i) { v[2 * i] = bf16_lo(p[i]); v[2 * i + 1] = bf16_hi(p[i]); }
    } else {
      const f32x4 p0 = *reinterpret_cast<const f32x4*>(static_cast<const float*>(src) + row * ld + col);
      const f32x4 p1 = *reinterpret_cast<const f32x4*>(static_cast<const float*>(src) + row * ld + col + 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) { v[i] = p0[i]; v[4 + i] = p1[i]; }
    }
  }
  const float am = group_max<4>(fmaxf(amax4(v[0], v[1], v[2], v[3]), amax4(v[4], v[5], v[6], v[7])));
  const unsigned byte = mx_scale_byte(am);
  const float mult = mx_multiplier(byte);
  if (valid) {
    *reinterpret_cast<u32x2*>(q + row * ldq + col) = u32x2{mx_pack4(v[0], v[1], v[2], v[3], mult, am == 0.f), mx_pack4(v[4], v[5], v[6], v[7], mult, am == 0.f)};
    if ((threadIdx.x & 3) == 0) sc[row * lds + (col >> 5)] = (u8)byte;
  }
}

// ---- ts_mx_layernorm_fwd: the row of w2v_layernorm_kernel (one wavefront per row, NV float4 per lane); a block is 8 consecutive lanes -------
template <int NV>
__global__ __launch_bounds__(256) void mx_layernorm_kernel(const float* __restrict__ x, const float* __restrict__ res, const float* __restrict__ xbias,
                                                           const float* __restrict__ w, const float* __restrict__ b, float* __restrict__ y,
                                                           long long rows, int c, float eps, u8* __restrict__ q, long long ldq, u8* __restrict__ sc,
                                                           long long lds) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* xr = x + row * c;
  const float* rr = res ? res + row * c : nullptr;
  float4 v[NV];
  float s = 0.f;
#pragma unroll
  for (int it = 0; it < NV; ++it) {
    const int i = (it * 64 + lane) * 4;
    v[it] = float4{0.f, 0.f, 0.f, 0.f};
    if (i < c) {
      v[it] = *reinterpret_cast<const float4*>(xr + i);
      if (rr) { const float4 r4 = *reinterpret_cast<const float4*>(rr + i); v[it].x += r4.x; v[it].y += r4.y; v[it].z += r4.z; v[it].w += r4.w; }
      if (xbias) { const float4 b4 = *reinterpret_cast<const float4*>(xbias + i); v[it].x += b4.x; v[it].y += b4.y; v[it].z += b4.z; v[it].w += b4.w; }
      s += (v[it].x + v[it].y) + (v[it].z + v[it].w);
    }
  }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  const float mu = s / c;
  float qs = 0.f;
#pragma unroll
  for (int it = 0; it < NV; ++it) {
    const int i = (it * 64 + lane) * 4;
    if (i < c) {
      const float d0 = v[it].x - mu, d1 = v[it].y - mu, d2 = v[it].z - mu, d3 = v[it].w - mu;
      qs += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    }
  }
  for (int o = 32; o > 0; o >>= 1) qs += __shfl_xor(qs, o);
  const float rs = rsqrtf(qs / c + eps);
#pragma unroll
  for (int it = 0; it < NV; ++it) {
    const int i = (it * 64 + lane) * 4;
    if (i < c) {                                  // c % 32 == 0: the 8 lanes of a block take this branch together
      const float4 w4 = *reinterpret_cast<const float4*>(w + i), b4 = *reinterpret_cast<const float4*>(b + i);
      const float4 o4 = float4{(v[it].x - mu) * rs * w4.x + b4.x, (v[it].y - mu) * rs * w4.y + b4.y, (v[it].z - mu) * rs * w4.z + b4.z,
                               (v[it].w - mu) * rs * w4.w + b4.w};
      if (y) *reinterpret_cast<float4*>(y + row * c + i) = o4;
      const float am = group_max<8>(amax4(o4.x, o4.y, o4.z, o4.w));
      const unsigned byte = mx_scale_byte(am);
      *reinterpret_cast<unsigned*>(q + row * ldq + i) = mx_pack4(o4.x, o4.y, o4.z, o4.w, mx_multiplier(byte), am == 0.f);
      if ((lane & 7) == 0) sc[row * lds + (i >> 5)] = (u8)byte;
    }
  }
}

// ---- ts_mx_pack_w ------------------------------------------------------------------------------------------------------
// one thread per 16 bytes of w_frag [n / 16][S][2][64][16]
__global__ __launch_bounds__(256) void mx_pack_w_kernel(const u8* __restrict__ wq, long long ldq, int N, int K, u8* __restrict__ out) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  const int S = K / MXK;
  if (g >= (long long)(N / 16) * S * 128) return;
  const int lane = (int)(g & 63), h = (int)((g >> 6) & 1);
  const long long f = g >> 7;
  const int s = (int)(f % S), nb = (int)(f / S);
  const u8* src = wq + (size_t)(16 * nb + (lane & 15)) * ldq + MXK * s + 64 * h + 16 * (lane >> 4);
  *reinterpret_cast<u32x4*>(out + g * 16) = *reinterpret_cast<const u32x4*>(src);
}
// one thread per dword of s_frag [ceil(n / 64)][S][64]
__global__ __launch_bounds__(256) void mx_pack_s_kernel(const u8* __restrict__ ws, long long lds, int N, int K, unsigned* __restrict__ out) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const int S = K / MXK, G = (N + 63) / 64;
  if (t >= (long long)G * S * 64) return;
  const int lane = (int)(t & 63);
  const long long f = t >> 6;
  const int s = (int)(f % S), g4 = (int)(f / S);
  unsigned d = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int nb = 4 * g4 + j;
    nb = nb < N / 16 ? nb : N / 16 - 1;
    d |= (unsigned)ws[(size_t)(16 * nb + (lane & 15)) * lds + 4 * s + (lane >> 4)] << (8 * j);
  }
  out[t] = d;
}

// ---- ts_mx_gemm_nt -------------------------------------------------------------------------------------------------------
struct MxArgs {
  const u8* xq;
  const u8* xs;
  const u8* wf;
  const unsigned* sf;
  const float* bias;
  float* y;
  unsigned short* y16;
  u8* yq;
  u8* ys;
  long long ldxq, ldxs, ldc, ld16, ldyq, ldys;
  int M, N, K, ep;
  int n_mt, n_nt;
};

// the 16-byte chunk c of a 128-byte LDS row sits at chunk c ^ mx_swz(row & 15): the 16-lane groups of a ds_read_b128 ({0-3, 12-15, 20-27}, ...)
// read rows {0-3, 12-15} at chunk g (+ 4) and rows 4-11 at chunk g ^ 1 (+ 4); rows of one parity share a 128-byte half of the bank row, so the
// table sends {0-3, 12-15} and {4-11} to the two halves of the chunk range, which the XOR with 1 keeps apart
__device__ __forceinline__ int mx_swz(int r) { return (int)((0x32765410u >> (4 * ((r >> 1) & 7))) & 7u); }

// EP: the epilogue, an instantiation each: tested at run time inside the unrolled accumulator loops it cost the GELU -> MX product a fifth of its time
template <int EP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void mx_gemm_kernel(const MxArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[MX_LDS];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  // workgroup -> tile: workgroup i runs on XCD i % 8; XCD x takes a contiguous range of the row-major tile walk (bijective for any tile count: the
  // first n % 8 XCDs take one tile more), so the column tiles of a row panel share that XCD's L2
  int mt_i, nt_i;
  {
    const int n_tiles = a.n_mt * a.n_nt;
    const int q = n_tiles >> 3, r = n_tiles & 7, xcd = blockIdx.x & 7, l = blockIdx.x >> 3;
    const int t = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + l;
    mt_i = t / a.n_nt;
    nt_i = t - mt_i * a.n_nt;
  }
  const int m0 = mt_i * MXM, n0 = nt_i * MXN;
  const int S = a.K / MXK;

  // A staging: thread -> rows (tid >> 3) + 32 q, chunk tid & 7 (a row's 128 bytes are 8 consecutive lanes: full cache lines, conflict-free writes).
  // Every operand is read through a buffer descriptor with a 32-bit offset (the launcher checks the extents)
  const auto rsrc = [](const void* p) { return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, 0x7fffffff, 0x00020000); };
  const __amdgpu_buffer_rsrc_t ra = rsrc(a.xq), rs = rsrc(a.xs), rb = rsrc(a.wf), rbs = rsrc(a.sf);
  const int srow = tid >> 3, schunk = tid & 7;
  int ao[4];
  const int wo0 = srow * MXK + ((schunk ^ mx_swz(srow & 15)) << 4);   // rows srow + 32 q share the swizzle (32 q % 16 == 0): + 32 q rows
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = srow + 32 * q;
    const long long m = m0 + r < a.M ? m0 + r : a.M - 1;
    ao[q] = (int)(m * a.ldxq) + 16 * schunk;
  }
  int so;
  {
    const int r = tid & (MXM - 1);
    const long long m = m0 + r < a.M ? m0 + r : a.M - 1;
    so = (int)(m * a.ldxs);
  }
  // B fragments: column blocks beyond N take the last valid one, their results are masked
  const int fr = lane & 15, fc = lane >> 4;
  int bo[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int nb = (n0 + wn * 64) / 16 + j;
    nb = nb < a.N / 16 ? nb : a.N / 16 - 1;
    bo[j] = nb * S * 2048 + lane * 16;
  }
  int bso;
  {
    int g4 = (n0 + wn * 64) / 64;
    g4 = g4 < (a.N + 63) / 64 ? g4 : (a.N + 63) / 64 - 1;
    bso = (g4 * S * 64 + lane) * 4;
  }
  const int fsw = mx_swz(fr);
  const int fa_lo = (wm * 64 + fr) * MXK + ((fc ^ fsw) << 4);   // K 16 fc ..; K 64 + 16 fc .. sits at chunk (4 + fc) ^ fsw: this offset ^ 64
  const int fs0 = 2 * MX_ABYTES + (wm * 64 + fr) * 4;

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  u32x4 ar[4];
  unsigned asr = 0;
  auto gload_a = [&](int s) {
#pragma unroll
    for (int q = 0; q < 4; ++q) ar[q] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(ra, ao[q], s * MXK, 0));
    asr = __builtin_amdgcn_raw_buffer_load_b32(rs, so, 4 * s, 0);     // threads t and t + 128 carry the same row's dword: no branch in the loop
  };
  auto lstore_a = [&](int buf) {
#pragma unroll
    for (int q = 0; q < 4; ++q) *reinterpret_cast<u32x4*>(smem + buf * MX_ABYTES + wo0 + q * 32 * MXK) = ar[q];
    *reinterpret_cast<unsigned*>(smem + 2 * MX_ABYTES + buf * MX_SBYTES + (tid & (MXM - 1)) * 4) = asr;
  };
  // the B fragments of the wave's four column blocks: ONE register set -- block j of step s + 1 is requested as soon as the four MFMAs that read
  // block j of step s have been issued, so its latency runs under the rest of this step, the barrier and the next step's fragment reads
  u32x4 bq[4][2];
  unsigned bs;
  auto gload_b = [&](int j, int s) {
#pragma unroll
    for (int h = 0; h < 2; ++h) bq[j][h] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rb, bo[j], s * 2048 + h * 1024, 0));
  };
  gload_a(0);
#pragma unroll
  for (int j = 0; j < 4; ++j) gload_b(j, 0);
  bs = __builtin_amdgcn_raw_buffer_load_b32(rbs, bso, 0, 0);
  lstore_a(0);
  __syncthreads();
  for (int s = 0; s < S; ++s) {
    const int buf = s & 1;
    const int sn = s + 1 < S ? s + 1 : s;       // the last step requests its own operands again: the loop body has no branch
    gload_a(sn);
    __builtin_amdgcn_sched_barrier(0);
    const char* const st = smem + buf * MX_ABYTES;
    i32x8 fa[4];
    int sa[4], sb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const u32x4 lo = *reinterpret_cast<const u32x4*>(st + fa_lo + i * 16 * MXK), hi = *reinterpret_cast<const u32x4*>(st + (fa_lo ^ 64) + i * 16 * MXK);
      const unsigned sd = *reinterpret_cast<const unsigned*>(smem + fs0 + buf * MX_SBYTES + i * 64);
      fa[i] = __builtin_bit_cast(i32x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
      sa[i] = (int)((sd >> (8 * fc)) & 0xffu);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) sb[j] = (int)((bs >> (8 * j)) & 0xffu);
    bs = __builtin_amdgcn_raw_buffer_load_b32(rbs, bso, sn * 256, 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const i32x8 fb = __builtin_bit_cast(i32x8, __builtin_shufflevector(bq[j][0], bq[j][1], 0, 1, 2, 3, 4, 5, 6, 7));
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fa[i], fb, acc[i][j], 0, 0, 0, sa[i], 0, sb[j]);
      __builtin_amdgcn_sched_barrier(0);
      gload_b(j, sn);
      __builtin_amdgcn_sched_barrier(0);
    }
    lstore_a(buf ^ 1);                          // the buffer every wave finished reading before the previous step's barrier
    __syncthreads();
  }

  // ---- epilogue: after the last step's barrier no wave reads the operand image any more ------------------------------------
  float* const ep = reinterpret_cast<float*>(smem + wave * 8192);
  const int erow = lane >> 3, ecol = (lane & 7) * 4;
#pragma unroll
  for (int jj = 0; jj < 2; ++jj) {
    const int nb = n0 + wn * 64 + 32 * jj;       // N % 32 == 0: a pass is entirely inside or outside [0, N)
    float bv[2];
#pragma unroll
    for (int jp = 0; jp < 2; ++jp) bv[jp] = (a.bias && nb < a.N) ? a.bias[nb + 16 * jp + fr] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int jp = 0; jp < 2; ++jp)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = acc[i][2 * jj + jp][r] + bv[jp];
          if constexpr (EP == TS_MX_EP_GELU_MX) v = gelu_erf(v);
          ep[(16 * i + 4 * fc + r) * 32 + 16 * jp + fr] = v;
        }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // wave-private tile: the row reads below follow the writes above
    if (nb < a.N) {
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int row = 8 * q + erow;
        const long long m = m0 + wm * 64 + row;
        if (m < a.M) {                           // the 8 lanes of a row segment (a quantisation block) take this branch together
          const f32x4 v = *reinterpret_cast<const f32x4*>(ep + row * 32 + ecol);
          if constexpr (EP == TS_MX_EP_BF16) {
            *reinterpret_cast<u32x2*>(a.y16 + m * a.ld16 + nb + ecol) = u32x2{pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3])};
          } else if constexpr (EP == TS_MX_EP_ACCUM) {
            float* const yp = a.y + m * a.ldc + nb + ecol;
            *reinterpret_cast<f32x4*>(yp) = *reinterpret_cast<const f32x4*>(yp) + v;
          } else {
            if (a.y) *reinterpret_cast<f32x4*>(a.y + m * a.ldc + nb + ecol) = v;
            const float am = group_max<8>(amax4(v[0], v[1], v[2], v[3]));
            const unsigned byte = mx_scale_byte(am);
            *reinterpret_cast<unsigned*>(a.yq + m * a.ldyq + nb + ecol) = mx_pack4(v[0], v[1], v[2], v[3], mx_multiplier(byte), am == 0.f);
            if ((lane & 7) == 0) a.ys[m * a.ldys + (nb >> 5)] = (u8)byte;
          }
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  }
}

}  // namespace

}  // namespace ts

using namespace ts;

extern "C" int ts_mxfp8_abi_version(void) { return TS_MXFP8_ABI_VERSION; }

extern "C" int ts_mx_quantize_rows(const void* src, int32_t src_bf16, int64_t ld_src, int64_t rows, int32_t k, void* q, int64_t ldq, void* scales,
                                   int64_t lds, void* stream_) {
  if (!src || !q || !scales || rows <= 0 || k <= 0 || ld_src < k || ldq < k || lds < (k + 31) / 32) return TS_EINVAL;
  if (k % 32 || ld_src % (src_bf16 ? 8 : 4) || ldq % 8 || misaligned(src) || misaligned(q, 7)) return TS_EUNSUPPORTED;
  if (rows * (k / 8) > 0x7fffffffll * 256) return TS_EUNSUPPORTED;
  TS_STREAM;
  const dim3 grid(nblk(rows * (k / 8)));
  if (src_bf16) hipLaunchKernelGGL(mx_quantize_kernel<true>, grid, dim3(256), 0, stream, src, (long long)ld_src, (long long)rows, k, static_cast<u8*>(q), (long long)ldq, static_cast<u8*>(scales), (long long)lds);
  else hipLaunchKernelGGL(mx_quantize_kernel<false>, grid, dim3(256), 0, stream, src, (long long)ld_src, (long long)rows, k, static_cast<u8*>(q), (long long)ldq, static_cast<u8*>(scales), (long long)lds);
  return hip_status(hipGetLastError());
}

extern "C" int ts_mx_layernorm_fwd(const float* x, const float* res, const float* xbias, const float* w, const float* b, float eps, int64_t rows,
                                   int32_t c, float* y, void* q, int64_t ldq, void* scales, int64_t lds, void* stream_) {
  if (!x || !w || !b || !q || !scales || rows <= 0 || c <= 0 || ldq < c || lds < (c + 31) / 32) return TS_EINVAL;
  if (c % 32 || c > 4096 || ldq % 4) return TS_EUNSUPPORTED;
  if (misaligned(x) || misaligned(res) || misaligned(xbias) || misaligned(w) || misaligned(b) || misaligned(y) || misaligned(q, 3)) return TS_EUNSUPPORTED;
  if ((rows + 3) / 4 > 0x7fffffffll) return TS_EUNSUPPORTED;
  TS_STREAM;
  const dim3 grid((unsigned)((rows + 3) / 4));
#define TS_MX_LN(NV_) hipLaunchKernelGGL(mx_layernorm_kernel<NV_>, grid, dim3(256), 0, stream, x, res, xbias, w, b, y, (long long)rows, c, eps, \
                                         static_cast<u8*>(q), (long long)ldq, static_cast<u8*>(scales), (long long)lds)
  if (c <= 512) TS_MX_LN(2); else if (c <= 1024) TS_MX_LN(4); else if (c <= 2048) TS_MX_LN(8); else TS_MX_LN(16);
#undef TS_MX_LN
  return hip_status(hipGetLastError());
}

extern "C" int64_t ts_mx_pack_w_scale_bytes(int32_t n, int32_t k) {
  if (n <= 0 || k <= 0 || n % 16 || k % MXK) return 0;
  return (int64_t)((n + 63) / 64) * (k / MXK) * 256;
}

extern "C" int ts_mx_pack_w(const void* wq, int64_t ldq, const void* ws, int64_t lds, int32_t n, int32_t k, void* w_frag, void* s_frag, void* stream_) {
  if (!wq || !ws || !w_frag || !s_frag || n <= 0 || k <= 0 || ldq < k || lds < (k + 31) / 32) return TS_EINVAL;
  if (n % 16 || k % MXK || ldq % 16 || misaligned(wq) || misaligned(w_frag) || misaligned(s_frag, 3)) return TS_EUNSUPPORTED;
  TS_STREAM;
  hipLaunchKernelGGL(mx_pack_w_kernel, dim3(nblk((long long)(n / 16) * (k / MXK) * 128)), dim3(256), 0, stream, static_cast<const u8*>(wq), (long long)ldq, n, k,
                     static_cast<u8*>(w_frag));
  hipLaunchKernelGGL(mx_pack_s_kernel, dim3(nblk((long long)((n + 63) / 64) * (k / MXK) * 64)), dim3(256), 0, stream, static_cast<const u8*>(ws), (long long)lds,
                     n, k, static_cast<unsigned*>(s_frag));
  return hip_status(hipGetLastError());
}

extern "C" int ts_mx_gemm_nt(const void* xq, int64_t ldxq, const void* xs, int64_t ldxs, const void* w_frag, const void* s_frag, const float* bias,
                             int32_t epilogue, float* y, int64_t ldc, void* y_bf16, int64_t ld16, void* yq, int64_t ldyq, void* ys, int64_t ldys,
                             int64_t rows, int32_t n, int32_t k, void* stream_) {
  if (!xq || !xs || !w_frag || !s_frag || rows <= 0 || n <= 0 || k <= 0 || ldxq < k || ldxs < (k + 31) / 32) return TS_EINVAL;
  if (epilogue == TS_MX_EP_BF16) {
    if (!y_bf16 || ld16 < n) return TS_EINVAL;
  } else if (epilogue == TS_MX_EP_ACCUM) {
    if (!y || ldc < n) return TS_EINVAL;
  } else if (epilogue == TS_MX_EP_GELU_MX) {
    if (!yq || !ys || ldyq < n || ldys < (n + 31) / 32 || (y && ldc < n)) return TS_EINVAL;
  } else {
    return TS_EINVAL;
  }
  if (n % 32 || k % MXK || ldxq % 16 || ldxs % 4 || misaligned(xq) || misaligned(xs, 3) || misaligned(w_frag) || misaligned(s_frag, 3) || misaligned(bias, 3))
    return TS_EUNSUPPORTED;
  if (epilogue == TS_MX_EP_BF16 && (ld16 % 4 || misaligned(y_bf16, 7))) return TS_EUNSUPPORTED;
  if (epilogue != TS_MX_EP_BF16 && y && (ldc % 4 || misaligned(y))) return TS_EUNSUPPORTED;
  if (epilogue == TS_MX_EP_GELU_MX && (ldyq % 4 || misaligned(yq, 3))) return TS_EUNSUPPORTED;
  const long long n_mt = (rows + MXM - 1) / MXM, n_nt = (n + MXN - 1) / MXN;
  // 32-bit buffer offsets of the operands
  if (n_mt * n_nt > 0x7fffffffll || rows * ldxq >= (1ll << 31) || rows * ldxs >= (1ll << 31) || (long long)n * k >= (1ll << 31)) return TS_EUNSUPPORTED;
  TS_STREAM;
  MxArgs a;
  a.xq = static_cast<const u8*>(xq); a.xs = static_cast<const u8*>(xs); a.wf = static_cast<const u8*>(w_frag); a.sf = static_cast<const unsigned*>(s_frag);
  a.bias = bias;
  a.y = epilogue == TS_MX_EP_BF16 ? nullptr : y;
  a.y16 = static_cast<unsigned short*>(y_bf16); a.yq = static_cast<u8*>(yq); a.ys = static_cast<u8*>(ys);
  a.ldxq = ldxq; a.ldxs = ldxs; a.ldc = ldc; a.ld16 = ld16; a.ldyq = ldyq; a.ldys = ldys;
  a.M = (int)rows; a.N = n; a.K = k; a.ep = epilogue;
  a.n_mt = (int)n_mt; a.n_nt = (int)n_nt;
  const dim3 grid((unsigned)(n_mt * n_nt));
  if (epilogue == TS_MX_EP_BF16) hipLaunchKernelGGL((mx_gemm_kernel<TS_MX_EP_BF16>), grid, dim3(256), 0, stream, a);
  else if (epilogue == TS_MX_EP_ACCUM) hipLaunchKernelGGL((mx_gemm_kernel<TS_MX_EP_ACCUM>), grid, dim3(256), 0, stream, a);
  else hipLaunchKernelGGL((mx_gemm_kernel<TS_MX_EP_GELU_MX>), grid, dim3(256), 0, stream, a);
  return hip_status(hipGetLastError());
}
