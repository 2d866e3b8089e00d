// Many MMS languages on one base (include_open/thunder_speech_amd/mms_lang_bank.h): every clip of a batch names, by a slot id read on the device,
// the language whose attention adapters and CTC head serve it.
//   ts_mms_lang_bank_adapter_fwd   ts_mms_attn_adapter_fwd (csrc/mms.hip) with the layer's six tensors taken from banks: mms_lang_adapter_kernel,
//                                  the same tile forward (ad_fwd_tile, csrc/mms_adapter_rows.hpp) on tiles that lie inside one clip
//   ts_mms_lang_bank_head_fwd      logits[b][v][f] = bias[s][v] + sum_k W[s][v][k] h[b][f][k] from the time-major encoder output: mms_lang_head_kernel
// In both a workgroup belongs to one clip (blockIdx.y), reads the clip's slot once and clamps an id outside the bank to slot 0, so every
// branch on the slot is uniform and no id can cause a read outside the banks.
#include "mms_adapter_rows.hpp"
#include "thunder_speech_amd/mms_lang_bank.h"

namespace ts {

// the clip's slot: ids[b], or 0 for an id outside [0, n_slots); the same value in every lane, kept scalar
__device__ __forceinline__ int bank_slot(const int* ids, int b, int n_slots) {
  const int s = ids[b];
  return __builtin_amdgcn_readfirstlane((unsigned)s < (unsigned)n_slots ? s : 0);
}

// ---------------------------------------------------------------------------------------------------------------------
// The adapter.  Grid (tiles of a clip, clip): tile x of clip b holds rows [16 x, 16 x + 16) of the clip; rows past the clip's end repeat the
// clip's last row and are never stored, as mms_adapter_kernel does at the end of the matrix.  p: the launch's arguments with every bank pointer
// at slot 0.  The tile shape per c is ad_tile_shape's, so a row's sums run in mms_adapter_kernel's order.
// ---------------------------------------------------------------------------------------------------------------------
struct AdBankArgs {
  AdArgs p;
  const int* ids;
  int n_slots, t;
};

template <int NQ, int NW, bool BF>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(AD_WAVES, AD_WAVES))) void mms_lang_adapter_kernel(const AdBankArgs q) {
  const int b = blockIdx.y;
  const int s = bank_slot(q.ids, b, q.n_slots);
  AdArgs p = q.p;
  const size_t sc = (size_t)s * p.c, sa = (size_t)s * p.a, sw = sc * p.a * (BF ? 2 : 4);
  p.norm_w += sc; p.norm_b += sc; p.b1 += sa; p.b2 += sc;
  p.w1 = static_cast<const char*>(p.w1) + sw;
  p.w2 = static_cast<const char*>(p.w2) + sw;
  const int r = blockIdx.x * 16 + (threadIdx.x & 15);
  const bool row_ok = r < q.t;
  ad_fwd_tile<NQ, NW, BF>(p, (long long)b * q.t + (row_ok ? r : q.t - 1), row_ok);
}

// ---------------------------------------------------------------------------------------------------------------------
// The head.  Grid (tiles of 16 frames of a clip, clip, groups of 256 classes); wave w of group z takes the class tiles (16 classes each)
// 16 z + w + 4 i, i < 4.  One 16 x 16 result tile: A = W (M = class), B = h^T (N = frame), so the accumulator of lane (rl, g) holds classes
// 4 g + 0..3 of frame rl and the 16 lanes of a group store 64 consecutive bytes of one class row.  The k loop reads the lane's own 8 (bf16) or
// 4 (f32) consecutive columns of its frame and of its class row: h is read from memory once per group of classes (the four waves read the same
// tile), W from L2.  Frames past the clip's end repeat the clip's last frame and are never stored.  No LDS, no barrier.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int HB_WAVES = 4, HB_TILES = 4;
constexpr float HB_NO_CLASS = -1e30f;

struct HeadBankArgs {
  const float* h;
  const void* w;
  const float* bias;
  const int *vocab, *ids;
  float* logits;
  int t, c, v_pad, n_slots, ldt;
};

template <bool BF>
__global__ __launch_bounds__(HB_WAVES * 64) void mms_lang_head_kernel(const HeadBankArgs p) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int rl = lane & 15, g = lane >> 4;
  const int b = blockIdx.y;
  const int nvt = p.v_pad / 16;
  const int vt0 = blockIdx.z * (HB_WAVES * HB_TILES) + wave;
  if (vt0 >= nvt) return;                                        // uniform
  const int s = bank_slot(p.ids, b, p.n_slots);
  const int c = p.c;
  const int f = blockIdx.x * 16 + rl;
  const bool f_ok = f < p.t;
  const float* hr = p.h + ((long long)b * p.t + (f_ok ? f : p.t - 1)) * c;
  const size_t w_row = ((size_t)s * p.v_pad + 16 * vt0 + rl) * c, w_step = (size_t)16 * HB_WAVES * c;
  f32x4 acc[HB_TILES];
#pragma unroll
  for (int i = 0; i < HB_TILES; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  if constexpr (BF) {
    const unsigned short* w = static_cast<const unsigned short*>(p.w) + w_row + 8 * g;       // k-step ks: columns 32 ks + 8 g + 0..7
    hr += 8 * g;
#pragma unroll 2
    for (int k = 0; k < c; k += 32) {
      const f32x4 x0 = *reinterpret_cast<const f32x4*>(hr + k), x1 = *reinterpret_cast<const f32x4*>(hr + k + 4);
      const s16x8 xb = __builtin_bit_cast(s16x8, uint4{pack_bf16(x0[0], x0[1]), pack_bf16(x0[2], x0[3]), pack_bf16(x1[0], x1[1]), pack_bf16(x1[2], x1[3])});
#pragma unroll
      for (int i = 0; i < HB_TILES; ++i) {
        if (vt0 + HB_WAVES * i >= nvt) break;                    // uniform
        const uint4 wf = *reinterpret_cast<const uint4*>(w + i * w_step + k);
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(s16x8, wf), xb, acc[i], 0, 0, 0);
      }
    }
  } else {
    const float* w = static_cast<const float*>(p.w) + w_row + 4 * g;                         // 16 columns a pass: MFMA r sums column 16 q + 4 g + r
    hr += 4 * g;
#pragma unroll 2
    for (int k = 0; k < c; k += 16) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(hr + k);
#pragma unroll
      for (int i = 0; i < HB_TILES; ++i) {
        if (vt0 + HB_WAVES * i >= nvt) break;
        const f32x4 w4 = *reinterpret_cast<const f32x4*>(w + i * w_step + k);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[r], x[r], acc[i], 0, 0, 0);
      }
    }
  }
  AD_MFMA_DRAIN;                                                 // the last MFMA ends the loop's block: its result is read by vector instructions below
  const int nv = min(p.vocab[s], p.v_pad);
  const float* bias = p.bias + (size_t)s * p.v_pad;
  float* out = p.logits + (long long)b * p.v_pad * p.ldt + f;
#pragma unroll
  for (int i = 0; i < HB_TILES; ++i) {
    const int v0 = 16 * (vt0 + HB_WAVES * i) + 4 * g;            // accumulator register r of lane (rl, g): class v0 + r, frame f
    if (vt0 + HB_WAVES * i >= nvt) break;                        // uniform
    const f32x4 b4 = *reinterpret_cast<const f32x4*>(bias + v0);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (f_ok) out[(long long)(v0 + r) * p.ldt] = v0 + r < nv ? acc[i][r] + b4[r] : HB_NO_CLASS;
  }
}

}  // namespace ts

using namespace ts;

extern "C" int ts_mms_lang_bank_abi_version(void) { return TS_MMS_LANG_BANK_ABI_VERSION; }

extern "C" int ts_mms_lang_bank_adapter_fwd(float* h, int32_t batch, int32_t t, int32_t c, int32_t a, const float* norm_w, const float* norm_b,
                                            const void* w1, const float* b1, const void* w2, const float* b2, int32_t n_slots, const int32_t* ids,
                                            const float* next_w, const float* next_b, float next_eps, float* y_next, void* y_next_op,
                                            int32_t precision, void* stream_) {
  if (n_slots <= 0 || !ids || batch <= 0 || t <= 0) return TS_EINVAL;
  if (const int st = ad_check_args(h, c, a, norm_w, norm_b, w1, b1, w2, b2, next_w, next_b, y_next, y_next_op, precision)) return st;
  if (batch > 65535 || misaligned(ids, 3)) return TS_EUNSUPPORTED;
  TS_STREAM;
  AdBankArgs q{};
  AdArgs& p = q.p;
  p.h = h; p.rows = (long long)batch * t; p.c = c; p.a = a; p.norm_w = norm_w; p.norm_b = norm_b; p.b1 = b1; p.b2 = b2; p.w1 = w1; p.w2 = w2;
  p.next_w = next_w; p.next_b = next_b; p.next_eps = next_eps;
  p.y_next = next_w ? y_next : nullptr; p.y_next16 = next_w ? static_cast<unsigned short*>(y_next_op) : nullptr;
  q.ids = ids; q.n_slots = n_slots; q.t = t;
  const dim3 grid((unsigned)(((long long)t + 15) / 16), (unsigned)batch);
  ad_tile_shape(c, [&](auto nq, auto nw) {
    constexpr int NQ = decltype(nq)::value, NW = decltype(nw)::value;
    if (precision) hipLaunchKernelGGL((mms_lang_adapter_kernel<NQ, NW, true>), grid, dim3(NW * 64), 0, stream, q);
    else hipLaunchKernelGGL((mms_lang_adapter_kernel<NQ, NW, false>), grid, dim3(NW * 64), 0, stream, q);
  });
  return hip_status(hipGetLastError());
}

extern "C" int ts_mms_lang_bank_head_fwd(const float* h, int32_t batch, int32_t t, int32_t c, const void* w_bank, const float* bias_bank,
                                         const int32_t* vocab, int32_t n_slots, int32_t v_pad, const int32_t* ids, float* logits, int32_t ldt,
                                         int32_t precision, void* stream_) {
  if (!h || !w_bank || !bias_bank || !vocab || !ids || !logits) return TS_EINVAL;
  if (batch <= 0 || t <= 0 || c <= 0 || n_slots <= 0 || v_pad <= 0 || ldt < t) return TS_EINVAL;
  if (c % 32 || v_pad % 16 || v_pad > 4096 || batch > 65535 || precision < 0 || precision > 1 || ldt % 4) return TS_EUNSUPPORTED;
  if (misaligned(h) || misaligned(w_bank) || misaligned(bias_bank) || misaligned(logits) || misaligned(vocab, 3) || misaligned(ids, 3))
    return TS_EUNSUPPORTED;
  TS_STREAM;
  HeadBankArgs p{};
  p.h = h; p.w = w_bank; p.bias = bias_bank; p.vocab = vocab; p.ids = ids; p.logits = logits;
  p.t = t; p.c = c; p.v_pad = v_pad; p.n_slots = n_slots; p.ldt = ldt;
  const int per_group = 16 * HB_WAVES * HB_TILES;
  const dim3 grid((unsigned)(((long long)t + 15) / 16), (unsigned)batch, (unsigned)((v_pad + per_group - 1) / per_group));
  if (precision) hipLaunchKernelGGL(mms_lang_head_kernel<true>, grid, dim3(HB_WAVES * 64), 0, stream, p);
  else hipLaunchKernelGGL(mms_lang_head_kernel<false>, grid, dim3(HB_WAVES * 64), 0, stream, p);
  return hip_status(hipGetLastError());
}
