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
// The attention adapter with the LayerNorm behind it.  The tile layout, the two matrix-core products, the LayerNorm statistics and the tile's
// forward itself (ad_fwd_tile) are csrc/mms_adapter_rows.hpp's (shared with the adapter's backward, csrc/mms_adapter_train.hip, and with the
// language bank, csrc/mms_lang_bank.hip).  A workgroup takes 16 consecutive rows of the flat [rows][c] matrix.
// p.in: the rows are read from there and written to p.h (the training forward, which keeps its input); NULL: in place on p.h.
// ---------------------------------------------------------------------------------------------------------------------
template <int NQ, int NW, bool BF>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(AD_WAVES, AD_WAVES))) void mms_adapter_kernel(const AdArgs p) {
  const long long row = (long long)blockIdx.x * 16 + (threadIdx.x & 15);
  const bool row_ok = row < p.rows;
  ad_fwd_tile<NQ, NW, BF>(p, row_ok ? row : p.rows - 1, row_ok);   // rows past the end: the last row again, never stored
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
  ad_tile_shape(c, [&](auto nq, auto nw) {
    constexpr int NQ = decltype(nq)::value, NW = decltype(nw)::value;
    if (precision) hipLaunchKernelGGL((mms_adapter_kernel<NQ, NW, true>), grid, dim3(NW * 64), 0, stream, p);
    else hipLaunchKernelGGL((mms_adapter_kernel<NQ, NW, false>), grid, dim3(NW * 64), 0, stream, p);
  });
  return hip_status(hipGetLastError());
}

extern "C" int ts_mms_attn_adapter_fwd(float* h, int64_t rows, int32_t c, int32_t a, const float* norm_w, const float* norm_b, const void* w1,
                                       const float* b1, const void* w2, const float* b2, const float* next_w, const float* next_b, float next_eps,
                                       float* y_next, void* y_next_op, int32_t precision, void* stream_) {
  if (rows <= 0) return TS_EINVAL;
  if (const int st = ad_check_args(h, c, a, norm_w, norm_b, w1, b1, w2, b2, next_w, next_b, y_next, y_next_op, precision)) return st;
  if ((rows + 15) / 16 > 0x7fffffffLL) return TS_EUNSUPPORTED;
  TS_STREAM;
  AdArgs p{};
  p.h = h; p.rows = rows; p.c = c; p.a = a; p.norm_w = norm_w; p.norm_b = norm_b; p.b1 = b1; p.b2 = b2; p.w1 = w1; p.w2 = w2;
  p.next_w = next_w; p.next_b = next_b; p.next_eps = next_eps;
  p.y_next = next_w ? y_next : nullptr; p.y_next16 = next_w ? static_cast<unsigned short*>(y_next_op) : nullptr;
  return adapter_launch(p, precision, stream);
}
