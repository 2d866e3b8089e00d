// What MMS (facebook/mms-1b-*) and XLS-R 1B need beyond the wav2vec2 launches (include/thunder_speech_amd/mms.h):
//   ts_mms_attention_fwd     the fused attention core at head_dim 80 (hidden 1280, 16 heads): w2v_flash_attn_kernel<80>, launched by attn_flash_launch
//                            (csrc/w2v_attn.hip; the head_dim 80 geometry and its LDS pitches are AttnGeom<80> of csrc/attn_tile.hpp)
//   ts_mms_attn_adapter_fwd  h += W2 relu(W1 LN(h) + b1) + b2 in place on the residual stream, with the LayerNorm that follows it: mms_adapter_kernel
// adapter_launch (declared in mms_adapter_rows.hpp) is that kernel's launcher, also used by ts_mms_attn_adapter_train_fwd (csrc/mms_adapter_train.hip).
#include "attn_tile.hpp"
#include "mms_adapter_rows.hpp"
#include "thunder_speech_amd/mms.h"

namespace ts {

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
  if (c / heads != 80 || misaligned(qkv) || misaligned(ctx) || heads > 65535 || batch > 65535) return TS_EUNSUPPORTED;
  TS_STREAM;
  return attn_flash_launch(80, qkv, batch, t, c, heads, key_len, ctx, stream);
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
