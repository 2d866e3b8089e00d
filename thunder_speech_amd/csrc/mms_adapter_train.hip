// The MMS attention adapter as a trainable node (include/thunder_speech_amd/mms_adapter_train.h):
//   ts_mms_attn_adapter_train_fwd   y = h + W2 relu(W1 LN(h) + b1) + b2 out of place: mms_adapter_kernel (csrc/mms.hip) reading h, writing y
//   ts_mms_attn_adapter_train_bwd   dh and the six parameter gradients from h and dy alone, in three launches:
//     1. mms_adapter_bwd_rows_kernel   16 rows per workgroup in the forward's tile layout (csrc/mms_adapter_rows.hpp).  It recomputes the row
//        statistics, u and z with the forward's code (the ReLU mask is the forward's, bit for bit), forms dz = (dy W2) . [z > 0] and -- unless
//        dh is NULL -- du = dz W1 and the LayerNorm backward.  du is formed twice, 32 columns at a time (once for the two row sums of the
//        LayerNorm backward, once for dh), so that only the h tile stays in registers: the budget is the forward's (a second [16][c] tile does not
//        fit 128 VGPRs at 10 chunks per wave, let alone at c = 4096).  The row's statistics, r and dz (width a) go to the workspace.
//     2. mms_adapter_bwd_cols_kernel   the sums over rows.  Workgroup = 64 columns x one range of rows x 16 adapter units; a lane owns a column,
//        the four waves take every fourth row and meet in LDS in a fixed order.  Per (row, column) it reads h and dy once (coalesced 256-byte
//        rows) and r / dz of the row as wave-uniform values, and accumulates d_w2, d_w1, d_b2 and -- with du of its column recomputed from dz and
//        W1's column -- d_norm_w and d_norm_b.  The contraction over rows is 3 a FMAs per element on the vector ALUs: with a <= 64 that stays
//        far below the time of the two loads, and it keeps the f32 sums over rows exact to the format with no operand shuffling.
//     3. mms_adapter_bwd_sum_kernel    the ordered sum of the row ranges' partial sums into the six gradients (set, not added).
// Why this decomposition: at the MMS-1B geometry (rows = 8 x 499, c = 1280) there are 250 row tiles, fewer than compute units, so per-workgroup
// partial sums of a persistent row grid would be one [2 a + 3][c] block PER TILE -- as many bytes as the tile itself.  Splitting the sums over
// rows off into a launch over column blocks lets the number of row ranges (at most 32) be chosen for the reduction alone.
// Bytes, next to the floor of 3 rows c 4 (read h, read dy, write dh): launch 1 reads h once and dy twice (the second time 80 KB per workgroup,
// just read: L2) and writes dh; launch 2 reads h and dy again (a / 16 times for a > 16); the partial sums are at most 32 (2 a + 3) c 4 bytes each
// way.  That is 5 rows c 4 from HBM for a = 16, 1.67 x the floor, against the 4 saved [rows][c] tensors plus their re-reads of an unfused
// LayerNorm / Linear / ReLU / Linear / add chain.
#include <type_traits>

#include "mms_adapter_rows.hpp"
#include "thunder_speech_amd/mms_adapter_train.h"

namespace ts {

__device__ __forceinline__ float round_bf16(float x) { return bf16_lo(pack_bf16(x, 0.f)); }

struct AbArgs {
  const float *h, *dy;
  float* dh;
  long long rows;
  int c, a;
  const float *norm_w, *norm_b, *b1;
  const void *w1, *w2;
  float *stats, *r, *dz;         // workspace: [rows][2] (mean, rstd), [rows][a], [rows][a]
};

template <int NQ, int NW, bool BF>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(AD_WAVES, AD_WAVES))) void mms_adapter_bwd_rows_kernel(const AbArgs p) {
  __shared__ float red[4][NW * 16];
  __shared__ __attribute__((aligned(16))) float zp[NW][16][AD_ZP];
  __shared__ float zs[16][AD_ZP];                                  // z of the tile, then dz
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rl = lane & 15, g = lane >> 4;
  const long long row0 = (long long)blockIdx.x * 16, row = row0 + rl;
  const bool row_ok = row < p.rows;
  const long long row_off = (row_ok ? row : p.rows - 1) * p.c;    // rows past the end: the last row again, never stored
  const float* hr = p.h + row_off;
  const float* dyr = p.dy + row_off;
  const int c = p.c, a = p.a;
  const int col0 = 16 * wave * NQ + 4 * g;
  f32x4 v[NQ];
  float mu, rs;
  ad_load_stats<NQ, NW>(hr, c, col0, v, red[0], red[1], wave, rl, g, mu, rs);
  if (wave == 0 && g == 0 && row_ok) {
    p.stats[2 * row] = mu;
    p.stats[2 * row + 1] = rs;
  }

  // ---- z = u W1^T + b1, as the forward; r = relu(z) to the workspace (rounded as the products will read it)
  ad_prod_in<NQ, NW, BF, false>([&](int i) { return ad_xhat(v[i], col0 + 16 * i, c, mu, rs, p.norm_w, p.norm_b); }, p.w1, c, a, wave, rl, g, col0, zp);
  __syncthreads();
  for (int idx = tid; idx < 16 * a; idx += NW * 64) {
    const int rr = idx / a, j = idx - rr * a;
    const float z = ad_zsum<NW>(zp, p.b1[j], rr, j);
    zs[rr][j] = z;
    const float r = fmaxf(z, 0.f);
    if (row0 + rr < p.rows) p.r[(row0 + rr) * a + j] = BF ? round_bf16(r) : r;
  }
  __syncthreads();

  // ---- dz = (dy W2) . [z > 0]
  ad_prod_in<NQ, NW, BF, true>(
      [&](int i) {
        const int col = col0 + 16 * i;
        return col < c ? *reinterpret_cast<const f32x4*>(dyr + col) : f32x4{0.f, 0.f, 0.f, 0.f};
      },
      p.w2, c, a, wave, rl, g, col0, zp);
  __syncthreads();
  for (int idx = tid; idx < 16 * a; idx += NW * 64) {
    const int rr = idx / a, j = idx - rr * a;
    float dz = zs[rr][j] > 0.f ? ad_zsum<NW>(zp, 0.f, rr, j) : 0.f;
    if (BF) dz = round_bf16(dz);
    zs[rr][j] = dz;
    if (row0 + rr < p.rows) p.dz[(row0 + rr) * a + j] = dz;
  }
  if (!p.dh) return;                                               // uniform: no upstream gradient wanted
  __syncthreads();

  // ---- du^T = W1^T dz^T, two chunks at a time; g = du . norm_w;  dh = dy + rs (g - mean(g) - xhat mean(g . xhat))
  auto dzval = [&](int j) -> float { return j < a ? zs[rl][j] : 0.f; };
  typename std::conditional<BF, s16x8[2], float[16]>::type zb;
  ad_out_b(dzval, g, zb);
  using WT = typename std::conditional<BF, unsigned short, float>::type;
  const WT* w1 = static_cast<const WT*>(p.w1);
  auto du2 = [&](int i, f32x4& e0, f32x4& e1) {                    // chunks i and i + 1 (zero where the wave's columns have ended)
    e0 = e1 = f32x4{0.f, 0.f, 0.f, 0.f};
    const int cm = 16 * (wave * NQ + i) + rl;
    if (cm - rl < c) e0 = ad_out_chunk<true>(e0, w1, cm, c, a, g, zb);
    if (cm + 16 - rl < c) e1 = ad_out_chunk<true>(e1, w1, cm + 16, c, a, g, zb);
    AD_MFMA_DRAIN;
  };
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int i = 0; i < NQ; i += 2) {
    f32x4 e[2];
    du2(i, e[0], e[1]);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int col = col0 + 16 * (i + k);
      if (col < c) {
        const f32x4 gk = e[k] * *reinterpret_cast<const f32x4*>(p.norm_w + col);
        const f32x4 xh = (v[i + k] - mu) * rs;
        const f32x4 gx = gk * xh;
        s1 += (gk[0] + gk[1]) + (gk[2] + gk[3]);
        s2 += (gx[0] + gx[1]) + (gx[2] + gx[3]);
      }
    }
  }
  const float m1 = ad_row_sum<NW>(s1, red[2], wave, rl, g) / c;
  const float m2 = ad_row_sum<NW>(s2, red[3], wave, rl, g) / c;
  float* dhr = p.dh + row_off;
#pragma unroll
  for (int i = 0; i < NQ; i += 2) {
    f32x4 e[2];
    du2(i, e[0], e[1]);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int col = col0 + 16 * (i + k);
      if (col < c && row_ok) {
        const f32x4 gk = e[k] * *reinterpret_cast<const f32x4*>(p.norm_w + col);
        const f32x4 xh = (v[i + k] - mu) * rs;
        *reinterpret_cast<f32x4*>(dhr + col) = *reinterpret_cast<const f32x4*>(dyr + col) + rs * (gk - m1 - xh * m2);
      }
    }
  }
}

// ---- the sums over rows ----
// Row ranges: at most 32, of at least 128 rows (a multiple of 4: the four waves of a workgroup take every fourth row)
struct AdSplit {
  int n;                  // ranges
  long long len;          // rows per range
};
static inline AdSplit ad_split(long long rows) {
  long long n = (rows + 127) / 128;
  if (n > 32) n = 32;
  const long long len = ((rows + n - 1) / n + 3) / 4 * 4;
  return AdSplit{(int)((rows + len - 1) / len), len};
}
// floats of one range's partial sums: d_w2 [c][a] | d_w1 [a][c] | d_norm_w [a / 16][c] | d_norm_b [a / 16][c] | d_b2 [c] | d_b1 [a]
static inline long long ad_part_floats(int c, int a) { return 2LL * c * a + 2LL * (a / 16) * c + c + a; }

struct AcArgs {
  const float *h, *dy, *stats, *r, *dz, *norm_w, *norm_b;
  const void* w1;
  float* part;
  long long rows, len, part_floats;
  int c, a;
};

constexpr int AC_VALS = 36;   // per column: 16 of d_w2, 16 of d_w1, d_norm_w, d_norm_b, d_b2; and d_b1 in lanes 0 .. 15

template <bool BF>
__global__ __launch_bounds__(256) void mms_adapter_bwd_cols_kernel(const AcArgs p) {
  __shared__ float comb[4][AC_VALS][64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = p.c, a = p.a;
  const int col = blockIdx.x * 64 + lane;
  const bool col_ok = col < c;
  const int cc = col_ok ? col : c - 1;
  const int zi = blockIdx.z, j0 = 16 * zi;
  const long long r0 = (long long)blockIdx.y * p.len;
  const long long r1 = r0 + p.len < p.rows ? r0 + p.len : p.rows;
  float w1c[16];
#pragma unroll
  for (int jj = 0; jj < 16; ++jj) {
    const size_t at = (size_t)(j0 + jj) * c + cc;
    w1c[jj] = BF ? bf16_to_f32(static_cast<const unsigned short*>(p.w1)[at]) : static_cast<const float*>(p.w1)[at];
  }
  const float nw = p.norm_w[cc], nb = p.norm_b[cc];
  float aw2[16], aw1[16], anw = 0.f, anb = 0.f, ab2 = 0.f, ab1 = 0.f;
#pragma unroll
  for (int jj = 0; jj < 16; ++jj) aw2[jj] = aw1[jj] = 0.f;
  // eight of the wave's rows per trip (row, row + 4, ...: the wave's order), their loads issued together: the trip is bound by their latency
  for (long long row = r0 + wave; row < r1; row += 32) {
    float hv[8], dv[8], mu[8], rs[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const long long rk = row + 4 * k < r1 ? row + 4 * k : row;
      mu[k] = p.stats[2 * rk]; rs[k] = p.stats[2 * rk + 1];
      hv[k] = p.h[rk * c + cc]; dv[k] = p.dy[rk * c + cc];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (row + 4 * k >= r1) break;                              // uniform
      const float xh = (hv[k] - mu[k]) * rs[k];
      float u = xh * nw + nb, dvr = dv[k];
      if (BF) { u = round_bf16(u); dvr = round_bf16(dvr); }
      const float* rr = p.r + (row + 4 * k) * a + j0;
      const float* dzr = p.dz + (row + 4 * k) * a + j0;
      float du = 0.f;
#pragma unroll
      for (int jj = 0; jj < 16; ++jj) {
        const float rj = rr[jj], dj = dzr[jj];
        aw2[jj] += dvr * rj;
        aw1[jj] += dj * u;
        du += dj * w1c[jj];
      }
      anw += du * xh;
      anb += du;
      ab2 += dv[k];
      ab1 += dzr[lane & 15];
    }
  }
#pragma unroll
  for (int jj = 0; jj < 16; ++jj) {
    comb[wave][jj][lane] = aw2[jj];
    comb[wave][16 + jj][lane] = aw1[jj];
  }
  comb[wave][32][lane] = anw;
  comb[wave][33][lane] = anb;
  comb[wave][34][lane] = ab2;
  comb[wave][35][lane] = ab1;
  __syncthreads();
  float* part = p.part + (long long)blockIdx.y * p.part_floats;
  const long long ca = (long long)c * a, zc = (long long)(a / 16) * c;
  for (int idx = tid; idx < AC_VALS * 64; idx += 256) {
    const int q = idx >> 6, l = idx & 63, ocol = blockIdx.x * 64 + l;
    const float s = ((comb[0][q][l] + comb[1][q][l]) + comb[2][q][l]) + comb[3][q][l];
    if (q == 35) {
      if (blockIdx.x == 0 && l < 16) part[2 * ca + 2 * zc + c + j0 + l] = s;
      continue;
    }
    if (ocol >= c) continue;
    if (q < 16) part[(long long)ocol * a + j0 + q] = s;
    else if (q < 32) part[ca + (long long)(j0 + q - 16) * c + ocol] = s;
    else if (q == 32) part[2 * ca + (long long)zi * c + ocol] = s;
    else if (q == 33) part[2 * ca + zc + (long long)zi * c + ocol] = s;
    else if (zi == 0) part[2 * ca + 2 * zc + ocol] = s;
  }
}

struct AsArgs {
  const float* part;
  float *d_w2, *d_w1, *d_norm_w, *d_norm_b, *d_b2, *d_b1;
  long long part_floats;
  int n, c, a;
};

__global__ __launch_bounds__(256) void mms_adapter_bwd_sum_kernel(const AsArgs p) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long ca = (long long)p.c * p.a, c = p.c;
  const int nz = p.a / 16;
  const long long zc = nz * c;
  float* dst;
  long long at;           // the first term's place in a range's partial sums
  int terms = 1;          // terms c apart per range (the blocks of 16 adapter units of d_norm_w / d_norm_b)
  if (t < ca) { dst = p.d_w2 + t; at = t; }
  else if (t < 2 * ca) { dst = p.d_w1 + (t - ca); at = t; }
  else if (t < 2 * ca + c) { dst = p.d_norm_w + (t - 2 * ca); at = t; terms = nz; }
  else if (t < 2 * ca + 2 * c) { dst = p.d_norm_b + (t - 2 * ca - c); at = 2 * ca + zc + (t - 2 * ca - c); terms = nz; }
  else if (t < 2 * ca + 3 * c) { dst = p.d_b2 + (t - 2 * ca - 2 * c); at = 2 * ca + 2 * zc + (t - 2 * ca - 2 * c); }
  else if (t < 2 * ca + 3 * c + p.a) { dst = p.d_b1 + (t - 2 * ca - 3 * c); at = 2 * ca + 2 * zc + c + (t - 2 * ca - 3 * c); }
  else return;
  // range by range, block by block; eight loads in flight, added in that order (an absent term adds 0)
  const int n = p.n * terms;
  float s = 0.f;
  for (int i0 = 0; i0 < n; i0 += 8) {
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int i = i0 + k, r = i / terms, z = i - r * terms;
      v[k] = i < n ? p.part[r * p.part_floats + at + z * c] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) s += v[k];
  }
  *dst = s;
}

// workspace layout, in floats (each part a multiple of 4 floats from the start)
struct AdWs {
  long long stats, r, dz, part, total;
};
static inline AdWs ad_workspace(long long rows, int c, int a) {
  AdWs w;
  w.stats = 0;
  w.r = (2 * rows + 3) / 4 * 4;
  w.dz = w.r + rows * a;
  w.part = w.dz + rows * a;
  w.total = w.part + ad_split(rows).n * ad_part_floats(c, a);
  return w;
}

static int adapter_train_refusal(int64_t rows, int32_t c, int32_t a, int32_t precision) {
  if (rows <= 0 || c <= 0 || a <= 0) return TS_EINVAL;
  if (a % 16 || a > 64 || c % 8 || c > 4096 || precision < 0 || precision > 1) return TS_EUNSUPPORTED;
  if ((rows + 15) / 16 > 0x7fffffffLL) return TS_EUNSUPPORTED;
  return TS_OK;
}

}  // namespace ts

using namespace ts;

extern "C" int ts_mms_adapter_train_abi_version(void) { return TS_MMS_ADAPTER_TRAIN_ABI_VERSION; }

extern "C" int ts_mms_attn_adapter_train_fwd(const float* h, int64_t rows, int32_t c, int32_t a, const float* norm_w, const float* norm_b,
                                             const void* w1, const float* b1, const void* w2, const float* b2, float* y, int32_t precision,
                                             void* stream_) {
  if (!h || !norm_w || !norm_b || !w1 || !b1 || !w2 || !b2 || !y) return TS_EINVAL;
  if (const int st = adapter_train_refusal(rows, c, a, precision)) return st;
  if (misaligned(h) || misaligned(norm_w) || misaligned(norm_b) || misaligned(w1) || misaligned(b1) || misaligned(w2) || misaligned(b2) || misaligned(y))
    return TS_EUNSUPPORTED;
  TS_STREAM;
  AdArgs p{};
  p.in = h; p.h = y; p.rows = rows; p.c = c; p.a = a; p.norm_w = norm_w; p.norm_b = norm_b; p.b1 = b1; p.b2 = b2; p.w1 = w1; p.w2 = w2;
  return adapter_launch(p, precision, stream);
}

extern "C" int64_t ts_mms_attn_adapter_train_bwd_workspace(int64_t rows, int32_t c, int32_t a) {
  if (rows <= 0 || c <= 0 || a <= 0) return TS_EINVAL;
  return ad_workspace(rows, c, a).total * 4;
}

extern "C" int ts_mms_attn_adapter_train_bwd(const float* h, const float* dy, int64_t rows, int32_t c, int32_t a, const float* norm_w,
                                             const float* norm_b, const void* w1, const float* b1, const void* w2, float* dh, float* d_norm_w,
                                             float* d_norm_b, float* d_w1, float* d_b1, float* d_w2, float* d_b2, void* workspace, int32_t precision,
                                             void* stream_) {
  if (!h || !dy || !norm_w || !norm_b || !w1 || !b1 || !w2 || !d_norm_w || !d_norm_b || !d_w1 || !d_b1 || !d_w2 || !d_b2 || !workspace)
    return TS_EINVAL;
  if (const int st = adapter_train_refusal(rows, c, a, precision)) return st;
  if (misaligned(h) || misaligned(dy) || misaligned(norm_w) || misaligned(norm_b) || misaligned(w1) || misaligned(b1) || misaligned(w2) ||
      misaligned(dh) || misaligned(d_norm_w) || misaligned(d_norm_b) || misaligned(d_w1) || misaligned(d_b1) || misaligned(d_w2) || misaligned(d_b2) ||
      misaligned(workspace))
    return TS_EUNSUPPORTED;
  TS_STREAM;
  const AdWs ws = ad_workspace(rows, c, a);
  float* wsf = static_cast<float*>(workspace);
  AbArgs p{};
  p.h = h; p.dy = dy; p.dh = dh; p.rows = rows; p.c = c; p.a = a; p.norm_w = norm_w; p.norm_b = norm_b; p.b1 = b1; p.w1 = w1; p.w2 = w2;
  p.stats = wsf + ws.stats; p.r = wsf + ws.r; p.dz = wsf + ws.dz;
  const dim3 grid((unsigned)((rows + 15) / 16));
#define TS_AB(NQ_, NW_)                                                                                                       \
  do {                                                                                                                        \
    if (precision) hipLaunchKernelGGL((mms_adapter_bwd_rows_kernel<NQ_, NW_, true>), grid, dim3(NW_ * 64), 0, stream, p);     \
    else hipLaunchKernelGGL((mms_adapter_bwd_rows_kernel<NQ_, NW_, false>), grid, dim3(NW_ * 64), 0, stream, p);              \
  } while (0)
  // the forward's tile shapes (adapter_launch, csrc/mms.hip)
  if (c <= 256) TS_AB(4, 4);
  else if (c <= 512) TS_AB(8, 4);
  else if (c <= 1024) TS_AB(8, 8);
  else if (c <= 1280) TS_AB(10, 8);
  else if (c <= 2048) TS_AB(8, 16);
  else TS_AB(16, 16);
#undef TS_AB
  if (const int st = hip_status(hipGetLastError())) return st;

  const AdSplit sp = ad_split(rows);
  AcArgs q{};
  q.h = h; q.dy = dy; q.stats = p.stats; q.r = p.r; q.dz = p.dz; q.norm_w = norm_w; q.norm_b = norm_b; q.w1 = w1; q.part = wsf + ws.part;
  q.rows = rows; q.len = sp.len; q.part_floats = ad_part_floats(c, a); q.c = c; q.a = a;
  const dim3 cgrid((c + 63) / 64, sp.n, a / 16);
  if (precision) hipLaunchKernelGGL(mms_adapter_bwd_cols_kernel<true>, cgrid, dim3(256), 0, stream, q);
  else hipLaunchKernelGGL(mms_adapter_bwd_cols_kernel<false>, cgrid, dim3(256), 0, stream, q);
  if (const int st = hip_status(hipGetLastError())) return st;

  AsArgs s{};
  s.part = q.part; s.d_w2 = d_w2; s.d_w1 = d_w1; s.d_norm_w = d_norm_w; s.d_norm_b = d_norm_b; s.d_b2 = d_b2; s.d_b1 = d_b1;
  s.part_floats = q.part_floats; s.n = sp.n; s.c = c; s.a = a;
  hipLaunchKernelGGL(mms_adapter_bwd_sum_kernel, dim3(nblk(2LL * c * a + 3LL * c + a)), dim3(256), 0, stream, s);
  return hip_status(hipGetLastError());
}
