// Fused self-attention for mixed-precision FINE-TUNING at head_dim 80 (XLS-R 1B / MMS: hidden 1280, 16 heads): the entry points of
// include/thunder_speech_amd/mms_train.h.  The contract is ts_w2v_attention_train_fwd / _bwd's with scale = 1 / sqrt(80), and so is the code: the
// head_dim 80 instantiations of attn_fwd_train_kernel / attn_bwd_dq_kernel / attn_bwd_dkv_kernel with attn_rowdot80_kernel, launched by
// attn_train_fwd_launch / attn_train_bwd_launch (csrc/w2v_attn_train.hip; the geometry is AttnGeom<80> of csrc/attn_tile.hpp).  What is this file's own
// are the argument checks, which differ from the head_dim 64 entry points' in what they refuse and with which code.
#include "attn_tile.hpp"
#include "thunder_speech_amd/mms_train.h"

using namespace ts;

static int mms_train_check(const void* qkv, int32_t batch, int32_t t, int32_t c, int32_t heads, float p_drop) {
  if (!qkv || batch <= 0 || t <= 0 || c <= 0 || heads <= 0 || c % heads || !(p_drop >= 0.f && p_drop < 1.f)) return TS_EINVAL;
  if (c / heads != 80 || misaligned(qkv) || heads > 65535 || batch > 65535 || (long long)batch * heads * t * t >= (1ll << 40)) return TS_EUNSUPPORTED;
  return TS_OK;
}

extern "C" int ts_mms_train_abi_version(void) { return TS_MMS_TRAIN_ABI_VERSION; }

/* see include/thunder_speech_amd/mms_train.h */
extern "C" int64_t ts_mms_attention_train_fwd_workspace(int32_t batch, int32_t t, int32_t c, int32_t heads) {
  return attn_train_fwd_workspace(batch, t, c, heads);
}

extern "C" int ts_mms_attention_train_fwd(const void* qkv_bf16, int32_t batch, int32_t t, int32_t c, int32_t heads, const int32_t* key_len, float p_drop,
                                          uint64_t seed, float* ctx, float* lse2, void* workspace, void* stream_) {
  if (int st = mms_train_check(qkv_bf16, batch, t, c, heads, p_drop)) return st;
  if (!ctx || !lse2 || (p_drop > 0.f && !workspace)) return TS_EINVAL;
  if (misaligned(ctx) || misaligned(lse2, 3) || misaligned(workspace) || misaligned(key_len, 3)) return TS_EUNSUPPORTED;
  TS_STREAM;
  return attn_train_fwd_launch(80, qkv_bf16, batch, t, c, heads, key_len, p_drop, seed, ctx, lse2, workspace, stream);
}

extern "C" int64_t ts_mms_attention_train_bwd_workspace(int32_t batch, int32_t t, int32_t c, int32_t heads) {
  return attn_train_bwd_workspace(batch, t, c, heads);
}

extern "C" int ts_mms_attention_train_bwd(const void* qkv_bf16, int32_t batch, int32_t t, int32_t c, int32_t heads, const int32_t* key_len, float p_drop,
                                          uint64_t seed, const float* dctx, const float* ctx, const float* lse2, const void* fwd_mask, float* dqkv,
                                          void* workspace, void* stream_) {
  if (int st = mms_train_check(qkv_bf16, batch, t, c, heads, p_drop)) return st;
  if (!dctx || !ctx || !lse2 || !dqkv || !workspace) return TS_EINVAL;
  if (misaligned(dctx) || misaligned(ctx) || misaligned(lse2, 3) || misaligned(dqkv) || misaligned(workspace) || misaligned(fwd_mask, 3) ||
      misaligned(key_len, 3))
    return TS_EUNSUPPORTED;
  TS_STREAM;
  return attn_train_bwd_launch(80, qkv_bf16, batch, t, c, heads, key_len, p_drop, seed, dctx, ctx, lse2, fwd_mask, dqkv, workspace, stream);
}
