// Shared device helpers for the thunder_speech_amd HIP kernels (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "thunder_speech_amd.h"

namespace ts {

typedef __attribute__((ext_vector_type(2))) short s16x2;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) int i32x4;

#define TS_LDS __attribute__((address_space(3)))

// float pair -> packed bf16 pair (round-to-nearest-even).  Compiler-scheduled form: safe right after an MFMA (hipcc pads
// the MFMA -> VALU hazard), but it lowers to two single conversions plus a v_perm_b32.
__device__ __forceinline__ unsigned pack_bf16(float lo, float hi) {
  bf16x2 v = {(__bf16)lo, (__bf16)hi};
  return __builtin_bit_cast(unsigned, v);
}
// ONE v_cvt_pk_bf16_f32.  hipcc inserts no wait states for inline asm, so the operands must NOT be the result of an
// MFMA issued within the last ~20 cycles (cdna_hip_programming.md 5.7 item 2); used by the epilogues only.
__device__ __forceinline__ unsigned pack_bf16_settled(float lo, float hi) {
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}
__device__ __forceinline__ float bf16_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf16_hi(unsigned u) { return __uint_as_float(u & 0xFFFF0000u); }
__device__ __forceinline__ float bf16_to_f32(unsigned short h) { return __uint_as_float(((unsigned)h) << 16); }

// keep the first `nv` bf16 elements of an 8-element group, zero the rest (nv may be <=0 or >=8)
__device__ __forceinline__ u32x4 keep_first(u32x4 v, int nv) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = nv - 2 * j;
    const unsigned m = r >= 2 ? 0xFFFFFFFFu : (r == 1 ? 0x0000FFFFu : 0u);
    v[j] &= m;
  }
  return v;
}

// Raw buffer descriptor (gfx9 layout) over [p, p + bytes): base, stride 0, num_records, 32-bit data format.
__device__ __forceinline__ i32x4 raw_rsrc(const void* p, unsigned bytes) {
  const unsigned long long a = reinterpret_cast<unsigned long long>(p);
  return i32x4{(int)(a & 0xffffffffu), (int)((a >> 32) & 0xffffu), (int)bytes, 0x00020000};
}
// Global -> LDS DMA of 16 bytes per lane (1 KiB per wave): lane L's 16 bytes at buffer offset voff + soff land at LDS byte
// address lds_dst + 16 L.  `after` is a register the DMA must be ordered behind: it is not read, it only pins the
// instruction below its producer.  hipcc orders the DMA against other MEMORY operations only, so without it the DMA
// that refills a tap slot floats above the MFMAs that consume the slot's old contents -- whose LDS reads may still be in
// flight -- and with an L2-hot source it lands first (measured: the taps of the last pass came from the next stage in
// 1-5 % of the waves).  Behind the last MFMA of the pass every read of the slot has returned.
// hipcc neither counts this operation in its vmcnt model nor orders LDS reads behind it: callers wait with vm_wait<>.
__device__ __forceinline__ void lds_dma16(i32x4 rsrc, const void* lds_dst, int voff, int soff, float after = 0.f) {
  const unsigned addr = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(TS_LDS const char*)lds_dst);
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
               :: "s"(addr), "v"(voff), "s"(rsrc), "s"(soff), "v"(after) : "memory");
}

// the sum / maximum over the 64 lanes of a wave, in every lane; V = float, or double (chan_reduce of csrc/train_bn.hip)
template <class V>
__device__ __forceinline__ V wave_sum(V v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

__host__ __device__ constexpr int round_up(int x, int m) { return (x + m - 1) / m * m; }

inline int hip_status(hipError_t e) { return e == hipSuccess ? TS_OK : (int)e; }

// ---- host side of the launchers ----
// first statements of a launcher taking `void* stream_`: the stream, and a clean error state for the hip_status(hipGetLastError()) it ends with
#define TS_STREAM hipStream_t stream = reinterpret_cast<hipStream_t>(stream_); (void)hipGetLastError()

static inline unsigned nblk(long long n) { return (unsigned)((n + 255) / 256); }       // 256-thread workgroups for n threads
// p is set and not aligned to mask + 1 bytes (a null pointer is an absent optional argument: aligned)
static inline bool misaligned(const void* p, uintptr_t mask = 15) { return p && (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

// The library's own GEMMs, called by the launchers of the other files.
// csrc/gemm_f32.hip: f32-accumulating GEMM on the f32 matrix-core instruction, any operand layout -- the f32 mode and the shapes without a kernel
// of their own
int gemm_f32(hipStream_t stream, bool in_bf16, const void* a, long long a_rs, long long a_cs, long long sa, long long ska, const void* b,
             long long b_rs, long long b_cs, long long sb, long long skb, void* c, long long ldc, long long sc, bool out_bf16, const float* bias,
             int M, int N, int K, int nkb, int batch, bool beta);
// csrc/gemm_nt.hip: token-major bf16 GEMM with the fused epilogue (bias, GELU, residual; _act: act 1 = GELU, 2 = SiLU)
int gemm_nt_bf16(hipStream_t stream, const void* x, long long lda, long long sx, const void* w, long long ldw, const float* bias,
                 const float* res, long long ld_res, float* y, long long ldc, void* y16, long long ld16, long long sy, long long M, int N, int K,
                 int gelu, int batch, const void* wf);
int gemm_nt_bf16_act(hipStream_t stream, const void* x, long long lda, long long sx, const void* w, long long ldw, const float* bias,
                     const float* res, long long ld_res, float* y, long long ldc, void* y16, long long ld16, long long sy, long long M, int N, int K,
                     int act, int batch, const void* wf);
// row-major y[M][N] (ldc) = x[M][K] (lda) W[N][K]^T (ldw) + beta y on gemm_f32, batched with element strides.  bf16 = x and W are bf16;
// y is f32 (or bf16 when y16 is set), accumulation f32 either way.
static inline int gemm_nt(hipStream_t stream, bool bf16, long long m, int n, int k, const void* x, long long lda, long long sx, const void* w,
                          long long ldw, long long sw, void* y, long long ldc, long long sy, float beta, int batch, bool y16 = false) {
  return gemm_f32(stream, bf16, x, lda, 1, sx, 0, w, 1, ldw, sw, 0, y, ldc, sy, y16, nullptr, (int)m, n, k, 1, batch, beta != 0.f);
}

// csrc/w2v_posconv.hip: out [B][T][C] f32 = grouped conv of src (bf16 operands) on the matrix-core positional-conv kernel, nothing added; c / groups == 64,
// `front` zero rows in front of each clip; the caller has checked the arguments (csrc/posconv_stack_train.hip)
int posconv_raw_conv(hipStream_t stream, const float* src, int batch, int t, int c, const void* w_taps_bf16, int kernel, int groups, int front, float* out,
                     void* workspace);

// compute units of the current device (one process per GPU: looked up once)
inline int cu_count() {
  static int n_cu = 0;
  if (n_cu) return n_cu;
  int dev = 0;
  hipDeviceProp_t prop;
  if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
    return n_cu = prop.multiProcessorCount;
  return n_cu = 256;
}

}  // namespace ts
