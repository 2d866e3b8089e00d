// A bank of LoRA adaptations behind one frozen base (include_staged/thunder_speech_amd/queued/lora_bank.h): ts_lora_bank_fwd adds, per clip, the
// low-rank terms of the slot that clip's id names to up to three target slices of y, one launch.  The base product stays the plan's GEMM; this
// launch runs behind it on the same buffer, as ts_lora_fwd does in training (csrc/lora_train.hip), and with its arithmetic: u rounded to bf16,
// both products on v_mfma_f32_16x16x32_bf16 at f32 accumulation.
//
// Decomposition (bf16 operands), lora_bank_kernel: grid = (row tiles of 16, clips), so a tile never straddles two clips and the slot is
// uniform over the workgroup; a workgroup whose id is outside [0, n_slots) returns before it reads anything else.  Workgroup = 16 rows x 8 waves.
//   phase 1  u[16][R] = x[16][k] Acat^T with Acat = [A_0; A_1; A_2] of the slot ([R][k], R = n_targets r, contiguous in the bank): x is read once
//            for all targets.  The 8 waves are KW splits of the contraction index x RW groups of NBW blocks of 16 rank indices (R <= 64: 8 x 1;
//            R = 96, 128: 4 x 2; R = 192: 2 x 4), 64 columns a trip; the KW partial tiles meet in LDS in a fixed order, are rounded to bf16 and
//            kept in LDS, one zero-padded [16][64] tile per target (a rank below 32 fills the k-step of phase 2 with zeros).
//   phase 2  per target: y^T[col][row] += s B_j[col][.] u_j[row][.], M = output column, N = row, contraction over the rank.  f32 y: 16 columns a
//            unit, the accumulator of lane (row, g) is columns 16 q + 4 g .. + 3 of its row (as csrc/lora_train.hip); bf16 y: 32 columns a unit,
//            two MFMAs whose rows of B_j are permuted so that lane (row, g) ends up with the 8 consecutive columns 32 q + 8 g .. + 7 of its row.
//            Either way the read-modify-write of y is one 16-byte load and store per lane and unit, the four lanes of a row cover 64
//            consecutive bytes, four units in flight per wave.
// f32 operands (lora_bank_f32_kernel): the same grid on the vector ALUs, a wave per (row, rank index) dot product over k with a butterfly sum
// over the lanes, then a thread per output element; fixed order too.  It serves precision="fp32" and tight checks, not speed.
//
// Bytes per launch next to the floor, q | v of the XLS-R 1B geometry at 16 x 20 s (rows = 15 984, k = n = 1280, r = 16, bf16 y): x 40.9 MB once +
// the read-modify-write of two bf16 slices 2 x 2 x 40.9 MB = 204.6 MB; the banks (8 slots: 1.3 MB) come out of L2 after their first read.
// Measured on an MI355X at that shape (profiles/lora_bank.md, tools/bench_lora_bank.py): 47.7 us against 25.7 us for its floor at 8 TB/s; the
// out_proj form (f32 y, one target) 38.2 us against 36.1 us for ts_lora_fwd on the same rows in the same run.
#include "ts_common.hpp"
#include "thunder_speech_amd/queued/lora_bank.h"

namespace ts {

constexpr int LB_NW = 8;       // waves of a workgroup
constexpr int LB_UP = 72;      // bf16 per row of a target's u tile in LDS (64 + 8: 16-byte rows)
constexpr int LB_RMAX = 192;   // 3 targets x rank 64
constexpr int LB_U = 4;        // units of output columns a wave keeps in flight in phase 2
// 16 wait states behind the last MFMA of a block before its result is read (see csrc/lora_train.hip LR_MFMA_DRAIN)
#define LB_MFMA_DRAIN                               \
  do {                                              \
    __builtin_amdgcn_sched_barrier(0);              \
    asm volatile("s_nop 15" ::: "memory");          \
    __builtin_amdgcn_sched_barrier(0);              \
  } while (0)

struct LbArgs {
  const void* x;             // [batch t][k], row pitch ldx
  const void* a;             // [n_slots][n_targets][r][k]
  const void* b;             // [n_slots][n_targets][n][r]
  const float* scales;       // [n_slots]
  const int* ids;            // [batch]
  void* y;                   // row pitch ldy
  long long ldx, ldy;
  int t, k, n, r, n_slots, n_targets, y_bf16;
  int col0, col1, col2;
};

// NBW: blocks of 16 rank indices per wave; RW: groups of such blocks the waves are split over (8 / RW splits of the contraction index);
// YB: y is bf16
template <int NBW, int RW, bool YB>
__global__ __launch_bounds__(LB_NW * 64) void lora_bank_kernel(const LbArgs p) {
  constexpr int KW = LB_NW / RW, NRB = NBW * RW, ZP = 16 * NRB + 4;
  __shared__ float zp[KW][16][ZP];
  __shared__ __attribute__((aligned(16))) unsigned short us[3][16][LB_UP];
  const int id = p.ids[blockIdx.y];
  if (id < 0 || id >= p.n_slots) return;                           // uniform: the base alone, nothing of the banks is read
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kw = wave / RW, rw = wave - kw * RW;
  const int rl = lane & 15, g = lane >> 4;
  const int k = p.k, r = p.r, n = p.n, R = p.n_targets * r;
  const int trow = (int)blockIdx.x * 16 + rl;                      // row inside the clip
  const bool row_ok = trow < p.t;
  const long long row = (long long)blockIdx.y * p.t + (row_ok ? trow : p.t - 1);     // rows past the clip's end: its last row again, never stored
  const unsigned short* xr = static_cast<const unsigned short*>(p.x) + row * p.ldx;
  const unsigned short* a = static_cast<const unsigned short*>(p.a) + (size_t)id * R * k;
  const unsigned short* b = static_cast<const unsigned short*>(p.b) + (size_t)id * p.n_targets * n * r;
  const float s = p.scales[id];
  for (int idx = tid; idx < p.n_targets * 16 * LB_UP; idx += LB_NW * 64) (&us[0][0][0])[idx] = 0;

  // ---- phase 1: this wave's columns and rank blocks of x . Acat^T
  f32x4 acc[NBW];
#pragma unroll
  for (int nb = 0; nb < NBW; ++nb) acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int base = 64 * kw; base < k; base += 64 * KW) {            // uniform
    const int col = base + 16 * g;
    const bool ok = col < k;                                       // k % 16 == 0: a lane's 16 columns are inside or outside together
    uint4 x0 = uint4{0u, 0u, 0u, 0u}, x1 = x0;
    if (ok) {
      x0 = *reinterpret_cast<const uint4*>(xr + col);
      x1 = *reinterpret_cast<const uint4*>(xr + col + 8);
    }
#pragma unroll
    for (int nb = 0; nb < NBW; ++nb) {
      const int j = 16 * (rw * NBW + nb) + rl;                     // B operand: this lane's row of Acat
      uint4 w0 = uint4{0u, 0u, 0u, 0u}, w1 = w0;
      if (ok && j < R) {
        const unsigned short* wr = a + (size_t)j * k + col;
        w0 = *reinterpret_cast<const uint4*>(wr);
        w1 = *reinterpret_cast<const uint4*>(wr + 8);
      }
      acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(s16x8, x0), __builtin_bit_cast(s16x8, w0), acc[nb], 0, 0, 0);
      acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(s16x8, x1), __builtin_bit_cast(s16x8, w1), acc[nb], 0, 0, 0);
    }
  }
  LB_MFMA_DRAIN;
  // accumulator register q of lane (n = rl, g): row 4 g + q, rank index 16 block + rl
#pragma unroll
  for (int nb = 0; nb < NBW; ++nb)
#pragma unroll
    for (int q = 0; q < 4; ++q) zp[kw][4 * g + q][16 * (rw * NBW + nb) + rl] = acc[nb][q];
  __syncthreads();
  for (int idx = tid; idx < 16 * 16 * NRB; idx += LB_NW * 64) {
    const int rr = idx / (16 * NRB), j = idx - rr * (16 * NRB);
    if (j >= R) continue;
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < KW; ++w) v += zp[w][rr][j];
    const int tj = j / r;
    us[tj][rr][j - tj * r] = (unsigned short)(pack_bf16(v, 0.f) & 0xFFFFu);
  }
  __syncthreads();

  // ---- phase 2, target by target: y^T[col][row] += s B_j[col][.] u_j[row][.], a unit = H MFMAs = 16 H output columns.  The MFMAs of a unit take
  // their rows of B_j permuted -- A-operand row i of MFMA h is column 16 H q + 4 H (i / 4) + 4 h + (i % 4) -- so that the accumulators of lane
  // (row, g), rows 4 g .. 4 g + 3 of each, are the 4 H consecutive columns 16 H q + 4 H g .. of its row: 16 bytes of y per lane and unit, H = 2
  // for bf16 y, H = 1 for f32 y (32 bytes per lane measured slower there: profiles/lora_bank.md)
  constexpr int H = YB ? 2 : 1;
  const int nq = n / (16 * H);
  const bool two = r > 32;                                         // uniform: a second k-step over the rank
  for (int tj = 0; tj < p.n_targets; ++tj) {                       // uniform
    const int c0 = tj == 0 ? p.col0 : (tj == 1 ? p.col1 : p.col2);
    const unsigned short* bt = b + (size_t)tj * n * r;
    const s16x8 zb0 = *reinterpret_cast<const s16x8*>(&us[tj][rl][8 * g]);
    const s16x8 zb1 = *reinterpret_cast<const s16x8*>(&us[tj][rl][32 + 8 * g]);
    float* yf = static_cast<float*>(p.y) + row * p.ldy + c0;
    unsigned short* yh = static_cast<unsigned short*>(p.y) + row * p.ldy + c0;
    for (int q0 = wave; q0 < nq; q0 += LB_U * LB_NW) {             // uniform
      f32x4 base[LB_U][H], d[LB_U][H];
#pragma unroll
      for (int u = 0; u < LB_U; ++u) {
        const int q = q0 + u * LB_NW;
#pragma unroll
        for (int h = 0; h < H; ++h) d[u][h] = base[u][h] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (q >= nq) continue;                                     // uniform
        const int cb = 16 * H * q + 4 * H * g;                     // this lane's 4 H columns of its row
        if constexpr (YB) {
          const uint4 raw = *reinterpret_cast<const uint4*>(yh + cb);
          base[u][0] = f32x4{bf16_lo(raw.x), bf16_hi(raw.x), bf16_lo(raw.y), bf16_hi(raw.y)};
          base[u][1] = f32x4{bf16_lo(raw.z), bf16_hi(raw.z), bf16_lo(raw.w), bf16_hi(raw.w)};
        } else {
          base[u][0] = *reinterpret_cast<const f32x4*>(yf + cb);
        }
#pragma unroll
        for (int h = 0; h < H; ++h) {
          const int cm = 16 * H * q + 4 * H * (rl >> 2) + 4 * h + (rl & 3);      // A operand: this lane's row of B_j (= output column)
          uint4 wf0 = uint4{0u, 0u, 0u, 0u}, wf1 = wf0;
          if (8 * g < r) wf0 = *reinterpret_cast<const uint4*>(bt + (size_t)cm * r + 8 * g);
          d[u][h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(s16x8, wf0), zb0, d[u][h], 0, 0, 0);
          if (two) {
            wf1 = *reinterpret_cast<const uint4*>(bt + (size_t)cm * r + 32 + 8 * g);
            d[u][h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(s16x8, wf1), zb1, d[u][h], 0, 0, 0);
          }
        }
      }
      LB_MFMA_DRAIN;
#pragma unroll
      for (int u = 0; u < LB_U; ++u) {
        const int q = q0 + u * LB_NW;
        if (q >= nq || !row_ok) continue;
        const int cb = 16 * H * q + 4 * H * g;
        if constexpr (YB) {
          const f32x4 v0 = base[u][0] + s * d[u][0], v1 = base[u][1] + s * d[u][1];
          *reinterpret_cast<uint4*>(yh + cb) = uint4{pack_bf16(v0[0], v0[1]), pack_bf16(v0[2], v0[3]), pack_bf16(v1[0], v1[1]), pack_bf16(v1[2], v1[3])};
        } else {
          *reinterpret_cast<f32x4*>(yf + cb) = base[u][0] + s * d[u][0];
        }
      }
    }
  }
}

// f32 operands: u in f32 in LDS, both products on the vector ALUs
__global__ __launch_bounds__(256) void lora_bank_f32_kernel(const LbArgs p) {
  __shared__ float uf[16][LB_RMAX + 1];
  const int id = p.ids[blockIdx.y];
  if (id < 0 || id >= p.n_slots) return;                           // uniform
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int k = p.k, r = p.r, n = p.n, R = p.n_targets * r;
  const int row0 = (int)blockIdx.x * 16;
  const int nrows = p.t - row0 < 16 ? p.t - row0 : 16;
  const long long grow0 = (long long)blockIdx.y * p.t + row0;
  const float* x = static_cast<const float*>(p.x) + grow0 * p.ldx;
  const float* a = static_cast<const float*>(p.a) + (size_t)id * R * k;
  const float* b = static_cast<const float*>(p.b) + (size_t)id * p.n_targets * n * r;
  const float s = p.scales[id];
  for (int pair = wave; pair < nrows * R; pair += 4) {             // uniform: one (row, rank index) per wave and trip
    const int rr = pair / R, j = pair - rr * R;
    const float* xr = x + (long long)rr * p.ldx;
    const float* ar = a + (size_t)j * k;
    float v = 0.f;
    for (int l = lane; l < k; l += 64) v += xr[l] * ar[l];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if (lane == 0) uf[rr][j] = v;
  }
  __syncthreads();
  const int width = p.n_targets * n;
  float* y = static_cast<float*>(p.y) + grow0 * p.ldy;
  for (int idx = tid; idx < nrows * width; idx += 256) {
    const int rr = idx / width, c = idx - rr * width;
    const int tj = c / n, i = c - tj * n;
    const int c0 = tj == 0 ? p.col0 : (tj == 1 ? p.col1 : p.col2);
    const float* br = b + ((size_t)tj * n + i) * r;
    const float* ur = &uf[rr][tj * r];
    float d = 0.f;
    for (int j = 0; j < r; ++j) d += ur[j] * br[j];
    float* out = y + (long long)rr * p.ldy + c0 + i;
    *out = *out + s * d;
  }
}

template <int NBW, int RW>
static void lora_bank_launch(const LbArgs& p, dim3 grid, hipStream_t stream) {
  if (p.y_bf16) hipLaunchKernelGGL((lora_bank_kernel<NBW, RW, true>), grid, dim3(LB_NW * 64), 0, stream, p);
  else hipLaunchKernelGGL((lora_bank_kernel<NBW, RW, false>), grid, dim3(LB_NW * 64), 0, stream, p);
}

}  // namespace ts

using namespace ts;

extern "C" int ts_lora_bank_abi_version(void) { return TS_LORA_BANK_ABI_VERSION; }

extern "C" int ts_lora_bank_fwd(const void* x, int32_t x_bf16, int64_t ldx, int32_t batch, int32_t t, int32_t k, const void* a_bank,
                                const void* b_bank, const float* scales, int32_t n_slots, int32_t n_targets, int32_t n, int32_t r,
                                const int32_t* ids, void* y, int32_t y_bf16, int64_t ldy, int32_t col0, int32_t col1, int32_t col2, void* stream_) {
  if (!x || !a_bank || !b_bank || !scales || !ids || !y) return TS_EINVAL;
  if (batch <= 0 || t <= 0 || k <= 0 || n <= 0 || r <= 0 || n_slots <= 0) return TS_EINVAL;
  if (n_targets < 1 || n_targets > 3) return TS_EINVAL;
  const int32_t col[3] = {col0, col1, col2};
  if (ldx < k) return TS_EINVAL;
  for (int j = 0; j < n_targets; ++j)
    if (col[j] < 0 || ldy < (int64_t)col[j] + n) return TS_EINVAL;
  if ((r != 8 && r != 16 && r != 32 && r != 64) || k % 32 || n % 32) return TS_EUNSUPPORTED;
  if (batch > 65535) return TS_EUNSUPPORTED;                       // one grid row per clip
  if (y_bf16 && !x_bf16) return TS_EUNSUPPORTED;
  for (int i = 0; i < n_targets; ++i)
    for (int j = i + 1; j < n_targets; ++j)
      if (col[i] < (int64_t)col[j] + n && col[j] < (int64_t)col[i] + n) return TS_EUNSUPPORTED;
  const int ya = y_bf16 ? 8 : 4;
  if (ldx % 8 || ldy % ya) return TS_EUNSUPPORTED;
  for (int j = 0; j < n_targets; ++j)
    if (col[j] % ya) return TS_EUNSUPPORTED;
  if (misaligned(x) || misaligned(a_bank) || misaligned(b_bank) || misaligned(y) || misaligned(scales, 3) || misaligned(ids, 3)) return TS_EUNSUPPORTED;
  TS_STREAM;
  LbArgs p{};
  p.x = x; p.a = a_bank; p.b = b_bank; p.scales = scales; p.ids = ids; p.y = y; p.ldx = ldx; p.ldy = ldy;
  p.t = t; p.k = k; p.n = n; p.r = r; p.n_slots = n_slots; p.n_targets = n_targets; p.y_bf16 = y_bf16 != 0;
  p.col0 = col0; p.col1 = n_targets > 1 ? col1 : 0; p.col2 = n_targets > 2 ? col2 : 0;
  const dim3 grid((unsigned)((t + 15) / 16), (unsigned)batch);
  if (!x_bf16) {
    hipLaunchKernelGGL(lora_bank_f32_kernel, grid, dim3(256), 0, stream, p);
    return hip_status(hipGetLastError());
  }
  switch ((n_targets * r + 15) / 16) {                             // blocks of 16 rank indices over all targets
    case 1: lora_bank_launch<1, 1>(p, grid, stream); break;
    case 2: lora_bank_launch<2, 1>(p, grid, stream); break;
    case 3: lora_bank_launch<3, 1>(p, grid, stream); break;
    case 4: lora_bank_launch<4, 1>(p, grid, stream); break;
    case 6: lora_bank_launch<3, 2>(p, grid, stream); break;
    case 8: lora_bank_launch<4, 2>(p, grid, stream); break;
    case 12: lora_bank_launch<3, 4>(p, grid, stream); break;
    default: return TS_EUNSUPPORTED;                               // unreachable for r in 8 / 16 / 32 / 64 and 1 .. 3 targets
  }
  return hip_status(hipGetLastError());
}
