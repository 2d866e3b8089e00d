// Audio classification heads (include_open/thunder_speech_amd/seq_cls.h): masked mean over time, projector, classifier, arg-max.
//   ts_seq_cls_pool   partials[b][s] (+)= w / len_b * sum of the frames of split s of clip b: seq_cls_pool_kernel, the HBM-bound launch
//   ts_seq_cls_head   seq_cls_rows_kernel twice (partials -> z, z -> logits: y[b][i] = bias[i] + W[i] . sum_s x[b][s]) and seq_cls_top_kernel
//                     (arg-max, its log-softmax, the arg-max restricted to the allowed classes)
// No launch uses an atomic or depends on the batch for its order of summation: a workgroup of the pool belongs to one (split, clip), every
// clip of a rows workgroup has accumulators of its own, the top launch has one workgroup per clip.
#include "ts_common.hpp"
#include "thunder_speech_amd/seq_cls.h"

namespace ts {

constexpr int SC_MAX_C = 4096, SC_MAX_P = 4096, SC_MAX_LABELS = 8192;
constexpr int SC_SPLIT_ROWS = 32;        // frames of a split, while that gives at most SC_MAX_SPLITS of them
constexpr int SC_MAX_SPLITS = 16;        // the head re-reads the partials once per tile of 64 projector rows: keep them few
constexpr int SC_POOL_UNROLL = 8;        // loads in flight per thread

// the split of t frames: a function of t alone (c only decides the workgroup's width)
struct PoolSplit {
  int splits, rows, block;
};
static inline PoolSplit pool_split(int t, int c) {
  int rows = SC_SPLIT_ROWS;
  if ((long long)rows * SC_MAX_SPLITS < t) rows = round_up((t + SC_MAX_SPLITS - 1) / SC_MAX_SPLITS, 8);
  return PoolSplit{(t + rows - 1) / rows, rows, round_up(c / 4, 64)};
}

// ---------------------------------------------------------------------------------------------------------------------
// The pool.  Grid (split, clip), c / 4 threads rounded up to whole waves: thread q sums channels 4 q + 0..3 over the split's valid frames in
// frame order, SC_POOL_UNROLL independent 16-byte loads at a time (a wave reads 1 KiB of one frame per instruction), scales by w / len and sets
// or adds its partial.  A split past the clip's length writes zeros (or adds nothing).
// ---------------------------------------------------------------------------------------------------------------------
struct PoolArgs {
  const float* h;
  const int* len;
  const float* w;
  float* partials;
  int t, c, splits, rows, accumulate;
};

__global__ __launch_bounds__(1024) void seq_cls_pool_kernel(const PoolArgs p) {
  const int q = threadIdx.x;
  if (4 * q >= p.c) return;
  const int b = blockIdx.y, s = blockIdx.x;
  int len = p.t;
  if (p.len) len = min(max(p.len[b], 0), p.t);
  const int r0 = s * p.rows, r1 = min(r0 + p.rows, len);
  const float* src = p.h + ((long long)b * p.t + r0) * p.c + 4 * q;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  int r = r0;
  for (; r + SC_POOL_UNROLL <= r1; r += SC_POOL_UNROLL, src += (long long)SC_POOL_UNROLL * p.c) {
    f32x4 x[SC_POOL_UNROLL];
#pragma unroll
    for (int u = 0; u < SC_POOL_UNROLL; ++u) x[u] = *reinterpret_cast<const f32x4*>(src + (long long)u * p.c);
#pragma unroll
    for (int u = 0; u < SC_POOL_UNROLL; ++u) acc += x[u];
  }
  for (; r < r1; ++r, src += p.c) acc += *reinterpret_cast<const f32x4*>(src);
  const float inv = len > 0 ? __fdiv_rn(1.f, (float)len) : 0.f;
  const float scale = p.w ? *p.w * inv : inv;
  f32x4* dst = reinterpret_cast<f32x4*>(p.partials + ((long long)b * p.splits + s) * p.c + 4 * q);
  f32x4 y = acc * scale;
  if (p.accumulate) y += *dst;
  *dst = y;
}

// ---------------------------------------------------------------------------------------------------------------------
// y[b][i] = bias[i] + sum_k W[i][k] x[b][k],  x[b][k] = sum_{s < ns} src[b][s][k] (s ascending).  Grid (tiles of SC_ROWS rows of W, groups of
// SC_CLIPS clips), 4 waves.  The workgroup first forms x of its clips in LDS (f32, up to 4 x 4096 values; every split's load issued before the
// first add, zeros for the clips past the batch), then a wave takes SC_RPI rows of the tile at a time: lane l multiplies each row's columns
// 4 (l + 64 m) + 0..3 (f32) or 8 (l + 64 m) + 0..7 (bf16, widened exactly) with every clip's x, m ascending -- the rows' loads are issued
// together and x is read from LDS once for them -- and the 64 lanes add up in wave_sum's butterfly.  A wave reads 1 KiB of a row per
// instruction; W is read once per group of clips.  Every (row, clip) has its own accumulator: a clip's result is the same whatever else is in
// the group.  Rows past n repeat row n - 1 and are not stored.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int SC_ROWS = 32, SC_CLIPS = 4, SC_WAVES = 4, SC_RPI = 4;

struct RowsArgs {
  const float* src;
  const void* w;
  const float* bias;
  float* y;
  int batch, ns, k, n;
};

// the lane's piece q of a row: 8 bf16 values widened exactly, or 4 f32 values
template <bool BF>
struct RowPiece {
  static constexpr int W = BF ? 8 : 4;
  float v[W];
  __device__ __forceinline__ void load(const void* row, int q) {
    if constexpr (BF) {
      const uint4 u = *reinterpret_cast<const uint4*>(static_cast<const unsigned short*>(row) + 8 * q);
      v[0] = bf16_lo(u.x); v[1] = bf16_hi(u.x); v[2] = bf16_lo(u.y); v[3] = bf16_hi(u.y);
      v[4] = bf16_lo(u.z); v[5] = bf16_hi(u.z); v[6] = bf16_lo(u.w); v[7] = bf16_hi(u.w);
    } else {
      const f32x4 u = *reinterpret_cast<const f32x4*>(static_cast<const float*>(row) + 4 * q);
      v[0] = u[0]; v[1] = u[1]; v[2] = u[2]; v[3] = u[3];
    }
  }
};

template <bool BF>
__global__ __launch_bounds__(SC_WAVES * 64) void seq_cls_rows_kernel(const RowsArgs p) {
  extern __shared__ __attribute__((aligned(16))) float sc_x[];          // [SC_CLIPS][k]
  constexpr int W = RowPiece<BF>::W;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b0 = blockIdx.y * SC_CLIPS;
  const int nb = min(SC_CLIPS, p.batch - b0);
  const int k = p.k, k4 = k / 4, ns = p.ns;
  for (int i = threadIdx.x; i < SC_CLIPS * k4; i += SC_WAVES * 64) {
    const int b = i / k4, q = i - b * k4;
    f32x4 x = {0.f, 0.f, 0.f, 0.f};
    if (b < nb) {
      const float* s = p.src + (long long)(b0 + b) * ns * k + 4 * q;
      f32x4 v[SC_MAX_SPLITS];
#pragma unroll
      for (int j = 0; j < SC_MAX_SPLITS; ++j)
        if (j < ns) v[j] = *reinterpret_cast<const f32x4*>(s + (long long)j * k);          // uniform
      x = v[0];
#pragma unroll
      for (int j = 1; j < SC_MAX_SPLITS; ++j)
        if (j < ns) x += v[j];
    }
    *reinterpret_cast<f32x4*>(sc_x + b * k + 4 * q) = x;
  }
  __syncthreads();
  const size_t row_bytes = (size_t)k * (BF ? 2 : 4);
  for (int r0 = blockIdx.x * SC_ROWS + wave * SC_RPI; r0 < min((int)(blockIdx.x + 1) * SC_ROWS, p.n); r0 += SC_WAVES * SC_RPI) {
    const char* rows[SC_RPI];
#pragma unroll
    for (int r = 0; r < SC_RPI; ++r) rows[r] = static_cast<const char*>(p.w) + (size_t)min(r0 + r, p.n - 1) * row_bytes;
    float acc[SC_RPI][SC_CLIPS];
#pragma unroll
    for (int r = 0; r < SC_RPI; ++r)
#pragma unroll
      for (int b = 0; b < SC_CLIPS; ++b) acc[r][b] = 0.f;
    for (int q = lane; W * q < k; q += 64) {
      RowPiece<BF> w[SC_RPI];
#pragma unroll
      for (int r = 0; r < SC_RPI; ++r) w[r].load(rows[r], q);
#pragma unroll
      for (int b = 0; b < SC_CLIPS; ++b) {
        float x[W];
#pragma unroll
        for (int e = 0; e < W; e += 4) {
          const f32x4 x4 = *reinterpret_cast<const f32x4*>(sc_x + b * k + W * q + e);
          x[e] = x4[0]; x[e + 1] = x4[1]; x[e + 2] = x4[2]; x[e + 3] = x4[3];
        }
#pragma unroll
        for (int r = 0; r < SC_RPI; ++r)
#pragma unroll
          for (int e = 0; e < W; ++e) acc[r][b] = fmaf(w[r].v[e], x[e], acc[r][b]);
      }
    }
#pragma unroll
    for (int r = 0; r < SC_RPI; ++r) {
      if (r0 + r >= p.n) break;                                          // uniform
      const float bias = p.bias[r0 + r];
#pragma unroll
      for (int b = 0; b < SC_CLIPS; ++b) {
        const float y = wave_sum(acc[r][b]) + bias;
        if (lane == 0 && b < nb) p.y[(long long)(b0 + b) * p.n + r0 + r] = y;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// One workgroup per clip over its n <= 8192 logits: the arg-max (lowest index on ties), the arg-max over the classes whose class_slot is not
// negative, and the arg-max's log-softmax: exp(x - max) of every class in parallel into LDS, then ONE thread adds them in class order.
// ---------------------------------------------------------------------------------------------------------------------
struct TopArgs {
  const float* logits;
  const int* class_slot;
  int* top1;
  float* logp;
  int* slot;
  int n;
};

struct Best {
  float v;
  int i;
};
__device__ __forceinline__ Best better(Best a, Best b) { return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a; }
__device__ __forceinline__ Best block_best(Best x, Best* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = better(x, Best{__shfl_xor(x.v, o), __shfl_xor(x.i, o)});
  __syncthreads();                                                       // sh may still be read from the previous reduction
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = x;
  __syncthreads();
  Best r = sh[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) r = better(r, sh[w]);
  return r;
}

__global__ __launch_bounds__(256) void seq_cls_top_kernel(const TopArgs p) {
  __shared__ __attribute__((aligned(16))) float e[SC_MAX_LABELS];
  __shared__ Best sh[4];
  const int b = blockIdx.x, n = p.n;
  const float* x = p.logits + (long long)b * n;
  const float NEG = -__builtin_huge_valf();
  Best all{NEG, 0x7fffffff}, allowed{NEG, 0x7fffffff};
  for (int v = threadIdx.x; v < n; v += 256) {
    const float xv = x[v];
    if (xv > all.v) all = Best{xv, v};                                   // v ascends within a thread: a tie keeps the lower index
    if (p.class_slot && p.class_slot[v] >= 0 && xv > allowed.v) allowed = Best{xv, v};
  }
  all = block_best(all, sh);
  if (all.i >= n) all = Best{x[0], 0};                                   // no finite-or-inf maximum (every logit a NaN): class 0
  if (p.class_slot) {
    allowed = block_best(allowed, sh);
    if (threadIdx.x == 0) p.slot[b] = allowed.i < n ? p.class_slot[allowed.i] : -1;
  }
  if (threadIdx.x == 0 && p.top1) p.top1[b] = all.i;
  if (!p.logp) return;
  for (int v = threadIdx.x; v < n; v += 256) e[v] = expf(x[v] - all.v);
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    {
#pragma clang fp reassociate(off)                                        // class order, whatever the build's fast-math flags allow
      int v = 0;
      for (; v + 4 <= n; v += 4) {
        const f32x4 e4 = *reinterpret_cast<const f32x4*>(e + v);
        s += e4[0]; s += e4[1]; s += e4[2]; s += e4[3];
      }
      for (; v < n; ++v) s += e[v];
    }
    p.logp[b] = -logf(s);                                                // x[top1] - max = 0
  }
}

}  // namespace ts

using namespace ts;

extern "C" int ts_seq_cls_abi_version(void) { return TS_SEQ_CLS_ABI_VERSION; }

static int pool_shape_status(int32_t t, int32_t c) {
  if (t <= 0 || c <= 0) return TS_EINVAL;
  if (c % 8 || c > SC_MAX_C) return TS_EUNSUPPORTED;
  return TS_OK;
}

extern "C" int ts_seq_cls_pool_launch_config(int32_t t, int32_t c, int32_t* splits, int32_t* rows_per_split, int32_t* block) {
  if (const int st = pool_shape_status(t, c)) return st;
  const PoolSplit s = pool_split(t, c);
  if (splits) *splits = s.splits;
  if (rows_per_split) *rows_per_split = s.rows;
  if (block) *block = s.block;
  return TS_OK;
}

extern "C" int64_t ts_seq_cls_pool_workspace_bytes(int32_t batch, int32_t t, int32_t c) {
  if (batch <= 0 || batch > 65535 || pool_shape_status(t, c)) return 0;
  return (int64_t)batch * pool_split(t, c).splits * c * (int64_t)sizeof(float);
}

extern "C" int ts_seq_cls_pool(const float* h, int32_t batch, int32_t t, int32_t c, const int32_t* len, const float* w, int32_t accumulate,
                               float* partials, void* stream_) {
  if (!h || !partials || batch <= 0 || accumulate < 0 || accumulate > 1) return TS_EINVAL;
  if (const int st = pool_shape_status(t, c)) return st;
  if (batch > 65535 || misaligned(h) || misaligned(partials) || misaligned(len, 3) || misaligned(w, 3)) return TS_EUNSUPPORTED;
  TS_STREAM;
  const PoolSplit s = pool_split(t, c);
  PoolArgs p{};
  p.h = h; p.len = len; p.w = w; p.partials = partials; p.t = t; p.c = c; p.splits = s.splits; p.rows = s.rows; p.accumulate = accumulate;
  hipLaunchKernelGGL(seq_cls_pool_kernel, dim3((unsigned)s.splits, (unsigned)batch), dim3((unsigned)s.block), 0, stream, p);
  return hip_status(hipGetLastError());
}

extern "C" int64_t ts_seq_cls_head_workspace_bytes(int32_t batch, int32_t p) {
  if (batch <= 0 || batch > 65535 || p <= 0 || p % 16 || p > SC_MAX_P) return 0;
  return (int64_t)batch * p * (int64_t)sizeof(float);
}

static void launch_rows(hipStream_t stream, bool bf16, const float* src, int ns, const void* w, const float* bias, float* y, int batch, int k, int n) {
  RowsArgs a{};
  a.src = src; a.w = w; a.bias = bias; a.y = y; a.batch = batch; a.ns = ns; a.k = k; a.n = n;
  const dim3 grid((unsigned)((n + SC_ROWS - 1) / SC_ROWS), (unsigned)((batch + SC_CLIPS - 1) / SC_CLIPS));
  const size_t lds = (size_t)SC_CLIPS * k * sizeof(float);              // at most 64 KiB (k <= 4096)
  if (bf16) hipLaunchKernelGGL(seq_cls_rows_kernel<true>, grid, dim3(SC_WAVES * 64), lds, stream, a);
  else hipLaunchKernelGGL(seq_cls_rows_kernel<false>, grid, dim3(SC_WAVES * 64), lds, stream, a);
}

extern "C" int ts_seq_cls_head(const float* partials, int32_t batch, int32_t t, int32_t c, const void* proj_w, const float* proj_b, int32_t p,
                               const void* cls_w, const float* cls_b, int32_t n_labels, const int32_t* class_slot, void* workspace, float* logits,
                               int32_t* top1, float* top1_logp, int32_t* slot, int32_t precision, void* stream_) {
  if (!partials || !proj_w || !proj_b || !cls_w || !cls_b || !workspace || !logits) return TS_EINVAL;
  if (batch <= 0 || p <= 0 || n_labels <= 0 || (class_slot == nullptr) != (slot == nullptr)) return TS_EINVAL;
  if (const int st = pool_shape_status(t, c)) return st;
  if (p % 16 || p > SC_MAX_P || n_labels > SC_MAX_LABELS || batch > 65535 || precision < 0 || precision > 1) return TS_EUNSUPPORTED;
  if (misaligned(partials) || misaligned(proj_w) || misaligned(cls_w) || misaligned(workspace)) return TS_EUNSUPPORTED;
  if (misaligned(proj_b, 3) || misaligned(cls_b, 3) || misaligned(class_slot, 3) || misaligned(logits, 3) || misaligned(top1, 3) ||
      misaligned(top1_logp, 3) || misaligned(slot, 3))
    return TS_EUNSUPPORTED;
  TS_STREAM;
  float* z = static_cast<float*>(workspace);
  launch_rows(stream, precision != 0, partials, pool_split(t, c).splits, proj_w, proj_b, z, batch, c, p);
  launch_rows(stream, precision != 0, z, 1, cls_w, cls_b, logits, batch, p, n_labels);
  TopArgs a{};
  a.logits = logits; a.class_slot = class_slot; a.top1 = top1; a.logp = top1_logp; a.slot = slot; a.n = n_labels;
  hipLaunchKernelGGL(seq_cls_top_kernel, dim3((unsigned)batch), dim3(256), 0, stream, a);
  return hip_status(hipGetLastError());
}
