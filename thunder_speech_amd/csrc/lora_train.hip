// The low-rank (LoRA) term of a frozen linear projection as a trainable node (include/thunder_speech_amd/lora_train.h), mixed precision:
//   ts_lora_fwd   u = x A^T, y += s u B^T into the target's column slice of the node's f32 result                  one launch
//   ts_lora_bwd   g = s dy B, dx += g A, dA = g^T x, dB = s dy^T u                                                   three launches
// The base product y = x W^T + b and dx = dy W stay the bf16 GEMM of csrc/gemm_nt.hip; these launches run behind it on the same buffers.
//
// Why the training forward keeps the low-rank path apart from W: forming W + s B A, rounding it to bf16 and running the ordinary GEMM would lose
// every delta below 2^-9 of a weight's magnitude in that rounding -- exactly the situation at the start of training (B = 0, then tiny): the
// forward would stop depending on B while the backward says it does.  Here x, A, B, u, g and dy are bf16 operands of products of their own, so
// the term s (x A^T) B^T reaches y at f32 accumulation whatever its size next to x W^T.  (Eval mode merges: huggingface/encoder.py.)
//
// Decomposition.  Both "rows" products are the same kernel, lora_rows_kernel: workgroup = 16 rows x 8 waves,
//   phase 1  mid[16][r] = s1 * in[16][kin] W1^T     W1 [r][kin]: the waves split the contraction index, 64 columns a trip each (a lane holds 16
//            consecutive bf16 of its row = two k-steps of v_mfma_f32_16x16x32_bf16; the order of a contraction is free), M = row, N = rank index;
//            the 8 partial tiles meet in LDS in a fixed order, are scaled, rounded to bf16 and kept in LDS (and stored: u16 / g)
//   phase 2  out[16][nout] += s2 * mid W2^T         W2 [nout][r]: M = output column, N = row, contraction over the rank (one k-step of 32, two for
//            r = 64; rank 8 and 16 fill the step with zeros), so the accumulator of lane (row, g) is columns 16 q + 4 g .. + 3 of its row: the
//            read-modify-write of out is one 16-byte load and store per lane and chunk, four chunks in flight per wave
//   forward:  in = x16, W1 = A, s1 = 1, mid = u16, W2 = B, out = the y slice (pitch ldy), s2 = s
//   backward: in = dy16 (pitch lddy), W1 = B^T, s1 = s, mid = g, W2 = A^T, out = dx, s2 = 1      (out = NULL: phase 1 only)
// The sums over rows (dA, dB) follow mms_adapter_bwd_cols_kernel / _sum_kernel (csrc/mms_adapter_train.hip): lora_bwd_cols_kernel has a lane own a
// column (of x16 for dA, of dy16 for dB), a workgroup = 64 columns x one range of rows x 16 rank indices (8 for r = 8), the four waves take every
// fourth row and meet in LDS in a fixed order; the other factor (g / u of the row) is wave-uniform.  r FMAs per element on the vector ALUs stay far
// below the time of the loads.  lora_bwd_sum_kernel adds the at most 32 row ranges' partial sums in order (dB scaled by s there).  No atomics.
//
// Bytes per launch next to the floor, at rows = 3 992, k = n = 1280, r = 16 (one target of the XLS-R 1B geometry at 8 x 10 s):
//   forward   floor: x16 10.2 MB + the read-modify-write of the f32 slice 2 x 20.4 MB = 51.1 MB.  The launch moves that plus u16 (0.13 MB) and
//             A, B (82 KB, re-read by the 250 workgroups out of L2): 1.00 x the floor; 0.33 GFLOP on the matrix cores.  Bound by the traffic.
//   backward  floor: dy16 10.2 MB + x16 10.2 MB + the read-modify-write of dx 40.9 MB = 61.3 MB.  The launches move: rows dy16 + dx (51.1 MB) + g
//             (0.26 MB); cols x16 + dy16 again (20.4 MB) + 32 ranges x r (k + n) 4 = 5.2 MB of partial sums, read back once by the sum: 82 MB,
//             1.34 x the floor (dy16's second read is the price of sums over rows in a launch of their own; r = 64 reads x16 / dy16 four times
//             there, out of L2 where they fit).
// One target per call: q and v of one node read x16 once each (10.2 MB a target more than a joint launch would, 20 % of the forward's floor).
// Measured on an MI355X at that shape (profiles/lora_finetune.md, tools/bench_lora.py): forward 12.9 us against 6.4 us for its floor at 8 TB/s;
// backward 37.3 us against 7.7 us, 28.6 us of it without dx -- the sums over rows are bound by the latency of their 2-byte loads, not by bytes.
#include "ts_common.hpp"
#include "thunder_speech_amd/lora_train.h"

namespace ts {

constexpr int LR_NW = 8;       // waves of a rows workgroup
constexpr int LR_ZP = 68;      // floats per row of a wave's partial mid tile (64 + 4)
constexpr int LR_UP = 72;      // bf16 per row of the mid tile in LDS (64 + 8: 16-byte rows)
// 16 wait states: more than an 8-pass MFMA's result needs before a vector / LDS / memory instruction may read it (see csrc/mms_adapter_rows.hpp:
// the compiler was seen to put no wait states between an MFMA that ends a basic block and a store that opens the next)
#define LR_MFMA_DRAIN                               \
  do {                                              \
    __builtin_amdgcn_sched_barrier(0);              \
    asm volatile("s_nop 15" ::: "memory");          \
    __builtin_amdgcn_sched_barrier(0);              \
  } while (0)

struct LrArgs {
  const unsigned short* in;      // [rows][kin] bf16, row pitch ldin
  const unsigned short* w1;      // [r][kin] bf16
  const unsigned short* w2;      // [nout][r] bf16
  unsigned short* mid16;         // [rows][r] bf16, or NULL
  float* midf;                   // [rows][r] f32 (the bf16-rounded values), or NULL
  float* out;                    // [rows][nout] f32, row pitch ldo, or NULL
  long long rows, ldin, ldo;
  int kin, nout, r;
  float s1, s2;
};

// NRB: blocks of 16 rank indices (r <= 16: 1); NKS: k-steps of 32 over the rank in phase 2
template <int NRB, int NKS>
__global__ __launch_bounds__(LR_NW * 64) void lora_rows_kernel(const LrArgs p) {
  __shared__ float zp[LR_NW][16][LR_ZP];
  __shared__ __attribute__((aligned(16))) unsigned short us[16][LR_UP];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rl = lane & 15, g = lane >> 4;
  const long long row0 = (long long)blockIdx.x * 16, row = row0 + rl;
  const bool row_ok = row < p.rows;
  const long long rr_ = row_ok ? row : p.rows - 1;                 // rows past the end: the last row again, never stored
  const unsigned short* inr = p.in + rr_ * p.ldin;
  const int kin = p.kin, r = p.r;
  for (int idx = tid; idx < 16 * LR_UP; idx += LR_NW * 64) (&us[0][0])[idx] = 0;

  // ---- phase 1: this wave's columns of in . W1^T
  f32x4 acc[NRB];
#pragma unroll
  for (int nb = 0; nb < NRB; ++nb) acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int base = 64 * wave; base < kin; base += 64 * LR_NW) {     // uniform
    const int col = base + 16 * g;
    const bool ok = col < kin;                                     // kin % 16 == 0: a lane's 16 columns are inside or outside together
    uint4 x0 = uint4{0u, 0u, 0u, 0u}, x1 = x0;
    if (ok) {
      x0 = *reinterpret_cast<const uint4*>(inr + col);
      x1 = *reinterpret_cast<const uint4*>(inr + col + 8);
    }
#pragma unroll
    for (int nb = 0; nb < NRB; ++nb) {
      const int j = 16 * nb + rl;                                  // B operand: this lane's W1 row
      uint4 w0 = uint4{0u, 0u, 0u, 0u}, w1 = w0;
      if (ok && j < r) {
        const unsigned short* wr = p.w1 + (size_t)j * kin + col;
        w0 = *reinterpret_cast<const uint4*>(wr);
        w1 = *reinterpret_cast<const uint4*>(wr + 8);
      }
      acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(s16x8, x0), __builtin_bit_cast(s16x8, w0), acc[nb], 0, 0, 0);
      acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(s16x8, x1), __builtin_bit_cast(s16x8, w1), acc[nb], 0, 0, 0);
    }
  }
  LR_MFMA_DRAIN;
  // accumulator register q of lane (n = rl, g): row 4 g + q, rank index 16 nb + rl
#pragma unroll
  for (int nb = 0; nb < NRB; ++nb)
#pragma unroll
    for (int q = 0; q < 4; ++q) zp[wave][4 * g + q][16 * nb + rl] = acc[nb][q];
  __syncthreads();
  for (int idx = tid; idx < 16 * 16 * NRB; idx += LR_NW * 64) {
    const int rr = idx / (16 * NRB), j = idx - rr * (16 * NRB);
    if (j >= r) continue;                                          // (rank 8: the upper half of the block stays zero)
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < LR_NW; ++w) t += zp[w][rr][j];
    const unsigned short h = (unsigned short)(pack_bf16(t * p.s1, 0.f) & 0xFFFFu);
    us[rr][j] = h;
    if (row0 + rr < p.rows) {
      if (p.mid16) p.mid16[(row0 + rr) * r + j] = h;
      if (p.midf) p.midf[(row0 + rr) * r + j] = bf16_to_f32(h);
    }
  }
  if (!p.out) return;                                              // uniform: no upstream gradient wanted
  __syncthreads();

  // ---- phase 2: out^T[col][row] += W2[col][.] mid[row][.]
  s16x8 zb[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) zb[ks] = *reinterpret_cast<const s16x8*>(&us[rl][32 * ks + 8 * g]);
  float* outr = p.out + rr_ * p.ldo;
  const int nq = p.nout / 16;
  for (int q0 = wave; q0 < nq; q0 += 4 * LR_NW) {                  // uniform
    f32x4 base[4], d[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = q0 + u * LR_NW;
      d[u] = base[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (q >= nq) continue;                                       // uniform
      base[u] = *reinterpret_cast<const f32x4*>(outr + 16 * q + 4 * g);
      const int cm = 16 * q + rl;                                  // A operand: this lane's W2 row (= output column)
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        const int j = 32 * ks + 8 * g;
        uint4 wf = uint4{0u, 0u, 0u, 0u};
        if (j < r) wf = *reinterpret_cast<const uint4*>(p.w2 + (size_t)cm * r + j);
        d[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(s16x8, wf), zb[ks], d[u], 0, 0, 0);
      }
    }
    LR_MFMA_DRAIN;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = q0 + u * LR_NW;
      if (q < nq && row_ok) *reinterpret_cast<f32x4*>(outr + 16 * q + 4 * g) = base[u] + p.s2 * d[u];
    }
  }
}

static void lora_rows_launch(const LrArgs& p, hipStream_t stream) {
  const dim3 grid((unsigned)((p.rows + 15) / 16)), block(LR_NW * 64);
  if (p.r <= 16) hipLaunchKernelGGL((lora_rows_kernel<1, 1>), grid, block, 0, stream, p);
  else if (p.r == 32) hipLaunchKernelGGL((lora_rows_kernel<2, 1>), grid, block, 0, stream, p);
  else hipLaunchKernelGGL((lora_rows_kernel<4, 2>), grid, block, 0, stream, p);
}

// ---- the sums over rows ----
// Row ranges: at most 32, of at least 128 rows (a multiple of 4: the four waves of a workgroup take every fourth row)
struct LrSplit {
  int n;                  // ranges
  long long len;          // rows per range
};
static inline LrSplit lr_split(long long rows) {
  long long n = (rows + 127) / 128;
  if (n > 32) n = 32;
  const long long len = ((rows + n - 1) / n + 3) / 4 * 4;
  return LrSplit{(int)((rows + len - 1) / len), len};
}

struct LcArgs {
  const unsigned short *x16, *dy16, *u16;
  const float* gf;
  float* part;            // per range: d_a [r][k] | d_b [n][r]
  long long rows, len, lddy, part_floats;
  int k, n, r, kblocks;
};

template <int JB>
__global__ __launch_bounds__(256) void lora_bwd_cols_kernel(const LcArgs p) {
  __shared__ float comb[4][JB][64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool second = (int)blockIdx.x >= p.kblocks;               // uniform: d_b's columns (of dy16), else d_a's (of x16)
  const int width = second ? p.n : p.k, r = p.r;
  const int colb = ((int)blockIdx.x - (second ? p.kblocks : 0)) * 64;
  const int cc = colb + lane < width ? colb + lane : width - 1;
  const unsigned short* v = second ? p.dy16 : p.x16;
  const long long ldv = second ? p.lddy : p.k;
  const int j0 = JB * blockIdx.z;
  const long long r0 = (long long)blockIdx.y * p.len;
  const long long r1 = r0 + p.len < p.rows ? r0 + p.len : p.rows;
  float a[JB];
#pragma unroll
  for (int jj = 0; jj < JB; ++jj) a[jj] = 0.f;
  // eight of the wave's rows per trip (row, row + 4, ...: the wave's order), their loads issued together
  for (long long row = r0 + wave; row < r1; row += 32) {
    float vv[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const long long rk = row + 4 * i < r1 ? row + 4 * i : row;
      vv[i] = bf16_to_f32(v[rk * ldv + cc]);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (row + 4 * i >= r1) break;                                // uniform
      const long long at = (row + 4 * i) * r + j0;
      if (second) {
#pragma unroll
        for (int h = 0; h < JB / 8; ++h) {
          const uint4 uu = *reinterpret_cast<const uint4*>(p.u16 + at + 8 * h);
          const unsigned w[4] = {uu.x, uu.y, uu.z, uu.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            a[8 * h + 2 * e] += vv[i] * bf16_lo(w[e]);
            a[8 * h + 2 * e + 1] += vv[i] * bf16_hi(w[e]);
          }
        }
      } else {
        const float* gr = p.gf + at;
#pragma unroll
        for (int jj = 0; jj < JB; ++jj) a[jj] += vv[i] * gr[jj];
      }
    }
  }
#pragma unroll
  for (int jj = 0; jj < JB; ++jj) comb[wave][jj][lane] = a[jj];
  __syncthreads();
  float* part = p.part + (long long)blockIdx.y * p.part_floats;
  for (int idx = tid; idx < JB * 64; idx += 256) {
    const int q = idx >> 6, l = idx & 63, ocol = colb + l;
    if (ocol >= width) continue;
    const float s = ((comb[0][q][l] + comb[1][q][l]) + comb[2][q][l]) + comb[3][q][l];
    if (second) part[(long long)r * p.k + (long long)ocol * r + j0 + q] = s;
    else part[(long long)(j0 + q) * p.k + ocol] = s;
  }
}

struct LsArgs {
  const float* part;
  float *d_a, *d_b;
  long long part_floats, ak;     // ak = r k: the first d_b element of a range's partial sums
  int n;                         // ranges
  float scale;
};

__global__ __launch_bounds__(256) void lora_bwd_sum_kernel(const LsArgs p) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= p.part_floats) return;
  // range by range; eight loads in flight, added in that order (an absent term adds 0)
  float s = 0.f;
  for (int i0 = 0; i0 < p.n; i0 += 8) {
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = i0 + i < p.n ? p.part[(i0 + i) * p.part_floats + t] : 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += v[i];
  }
  if (t < p.ak) p.d_a[t] = s;
  else p.d_b[t - p.ak] = p.scale * s;
}

// workspace layout, in floats (each part a multiple of 4 floats from the start)
struct LrWs {
  long long g, part, total;
};
static inline LrWs lr_workspace(long long rows, int k, int n, int r) {
  LrWs w;
  w.g = 0;
  w.part = (rows * r + 3) / 4 * 4;
  w.total = w.part + lr_split(rows).n * (long long)r * ((long long)k + n);
  return w;
}

static int lora_refusal(int64_t rows, int32_t k, int32_t n, int32_t r) {
  if (rows <= 0 || k <= 0 || n <= 0 || r <= 0) return TS_EINVAL;
  if ((r != 8 && r != 16 && r != 32 && r != 64) || k % 32 || n % 32) return TS_EUNSUPPORTED;
  if (rows > 16LL * 0x7fffffffLL) return TS_EUNSUPPORTED;          // one workgroup per 16 rows in grid x
  return TS_OK;
}

}  // namespace ts

using namespace ts;

extern "C" int ts_lora_abi_version(void) { return TS_LORA_ABI_VERSION; }

extern "C" int ts_lora_fwd(const void* x16, int64_t rows, int32_t k, const void* a16, const void* b16, int32_t n, int32_t r, float scale, float* y,
                           int64_t ldy, void* u16, void* stream_) {
  if (!x16 || !a16 || !b16 || !y || !u16) return TS_EINVAL;
  if (const int st = lora_refusal(rows, k, n, r)) return st;
  if (ldy < n) return TS_EINVAL;
  if (ldy % 4 || misaligned(x16) || misaligned(a16) || misaligned(b16) || misaligned(y) || misaligned(u16)) return TS_EUNSUPPORTED;
  TS_STREAM;
  LrArgs p{};
  p.in = static_cast<const unsigned short*>(x16); p.ldin = k; p.kin = k; p.w1 = static_cast<const unsigned short*>(a16); p.s1 = 1.f;
  p.mid16 = static_cast<unsigned short*>(u16); p.w2 = static_cast<const unsigned short*>(b16); p.out = y; p.ldo = ldy; p.nout = n; p.s2 = scale;
  p.rows = rows; p.r = r;
  lora_rows_launch(p, stream);
  return hip_status(hipGetLastError());
}

extern "C" int64_t ts_lora_bwd_workspace(int64_t rows, int32_t k, int32_t n, int32_t r) {
  if (const int st = lora_refusal(rows, k, n, r)) return st;
  return lr_workspace(rows, k, n, r).total * 4;
}

extern "C" int ts_lora_bwd(const void* dy16, int64_t lddy, const void* x16, const void* u16, int64_t rows, int32_t k, int32_t n, int32_t r, float scale,
                           const void* at16, const void* bt16, float* dx, float* d_a, float* d_b, void* workspace, void* stream_) {
  if (!dy16 || !x16 || !u16 || !at16 || !bt16 || !d_a || !d_b || !workspace) return TS_EINVAL;
  if (const int st = lora_refusal(rows, k, n, r)) return st;
  if (lddy < n) return TS_EINVAL;
  if (lddy % 8 || misaligned(dy16) || misaligned(x16) || misaligned(u16) || misaligned(at16) || misaligned(bt16) || misaligned(dx) || misaligned(d_a) ||
      misaligned(d_b) || misaligned(workspace))
    return TS_EUNSUPPORTED;
  TS_STREAM;
  const LrWs ws = lr_workspace(rows, k, n, r);
  float* wsf = static_cast<float*>(workspace);
  LrArgs p{};
  p.in = static_cast<const unsigned short*>(dy16); p.ldin = lddy; p.kin = n; p.w1 = static_cast<const unsigned short*>(bt16); p.s1 = scale;
  p.midf = wsf + ws.g; p.w2 = static_cast<const unsigned short*>(at16); p.out = dx; p.ldo = k; p.nout = k; p.s2 = 1.f;
  p.rows = rows; p.r = r;
  lora_rows_launch(p, stream);
  if (const int st = hip_status(hipGetLastError())) return st;

  const LrSplit sp = lr_split(rows);
  LcArgs q{};
  q.x16 = static_cast<const unsigned short*>(x16); q.dy16 = p.in; q.u16 = static_cast<const unsigned short*>(u16); q.gf = p.midf;
  q.part = wsf + ws.part; q.rows = rows; q.len = sp.len; q.lddy = lddy; q.part_floats = (long long)r * ((long long)k + n);
  q.k = k; q.n = n; q.r = r; q.kblocks = (k + 63) / 64;
  const int jb = r == 8 ? 8 : 16;
  const dim3 cgrid(q.kblocks + (n + 63) / 64, sp.n, r / jb);
  if (jb == 8) hipLaunchKernelGGL(lora_bwd_cols_kernel<8>, cgrid, dim3(256), 0, stream, q);
  else hipLaunchKernelGGL(lora_bwd_cols_kernel<16>, cgrid, dim3(256), 0, stream, q);
  if (const int st = hip_status(hipGetLastError())) return st;

  LsArgs s{};
  s.part = q.part; s.d_a = d_a; s.d_b = d_b; s.part_floats = q.part_floats; s.ak = (long long)r * k; s.n = sp.n; s.scale = scale;
  hipLaunchKernelGGL(lora_bwd_sum_kernel, dim3(nblk(s.part_floats)), dim3(256), 0, stream, s);
  return hip_status(hipGetLastError());
}
