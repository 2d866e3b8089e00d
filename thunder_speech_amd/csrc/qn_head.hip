// The end of a QuartzNet forward pass as one launch (gfx950): the encoder's last block -- a 1x1 convolution with folded BatchNorm and ReLU,
// 512 -> 1024 channels (reference quartznet/blocks.py:389 in body()) -- and the conv1d CTC decoder behind it (blocks.py:199-216, 1024 -> 29).
//
//   h[b, c, t]      = bf16(relu(b17[c] + sum_k W17[c, k] x[b, k, t]))          (0 from len[b] on, when lengths are given)
//   logits[b, v, t] = bd[v] + sum_c Wd[v, c] h[b, c, t]
//
// As two launches (csrc/tcs_split.hip, csrc/pw_logits.hip) h is 98 MB written and 98 MB read back per 64 x 15 s step to make 5.6 MB of logits.
// Here it never leaves the registers:
//   workgroup = (clip, 96-frame tile), 8 waves at up to 256 VGPRs, one workgroup per CU, persistent over tiles in the split kernel's
//     XCD-contiguous order.  The [c_in][96] tile of x is fetched ONCE into LDS (16 B per lane; the split kernel's XOR-swizzled 256-byte rows);
//     the next tile's rows are requested before the current tile's partial sums meet and wait in registers meanwhile.
//   GEMM1, transposed: hT[c][t] = W17[c][:] x[:][t] on v_mfma_f32_16x16x32_bf16.  Wave w owns hidden channels [512 p + 64 w, + 64) in pass p:
//     A = the weight fragments ts_tcs_subblock_fwd already uses (operands swapped: the B fragments of D[t][co] are the A fragments of D[co][t]),
//     streamed from L2 through a register ring three k-steps deep that runs on across passes and tiles; B = x fragments read out of the tile with
//     ds_read_b64_tr_b16, the split kernel's consumer access.  The shift is the initial accumulator and k ascends, as in the split kernel.
//   GEMM2 without an LDS round trip: in the transposed form a lane's four accumulators of a 16-channel tile are (frame lane & 15, channels
//     4 kg .. 4 kg + 3).  Two such tiles -- ReLU'd, masked, packed to bf16 -- ARE a B fragment of logitsT[v][t] += Wd[v][c] hT[c][t], provided the
//     k-order of the Wd fragments follows (plan.pack_head_wd): the S -> P step of the fused attention kernels (csrc/attn_tile.hpp).
//   Each wave keeps 32 x 96 partial logits (48 registers) over all passes; at the end of a tile the eight partial sums meet through the then
//     idle x tile in wave order (wave 0's carries bd).  No atomics.
#include "tcs_shared.hpp"
#include "thunder_speech_amd/qn_head.h"

#include <atomic>

namespace ts {

namespace {

constexpr int HT = TS_QN_HEAD_TILE;           // frames per tile
constexpr int HROWB = 256;                    // bytes per staged channel row
constexpr int HMT = HT / 16;                  // 16-frame accumulator tiles
constexpr int HNT = 4;                        // 16-channel accumulator tiles per wave and pass
constexpr int HWAVES = 8;
constexpr int HRING = 3;                      // k-steps of weight fragments in flight
constexpr int HNX = TS_QN_HEAD_CIN_MAX * (HT / 8) / (64 * HWAVES);      // 16-byte row chunks per thread and tile: 8 + 4
constexpr int HPART = HMT * 2 * 64 * 16;      // bytes of a wave's partial logits

struct HeadArgs {
  const unsigned short* x; const int* len; const unsigned short* w17; const float* b17; const unsigned short* wd; const float* bd; float* y;
  int batch, c_in, hidden, n_classes, t_out, pitch_in, pitch_out, n_tt, n_tiles, xcd, lds_main;
};

__global__ __launch_bounds__(64 * HWAVES) void qn_head_kernel(const HeadArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];             // max([c_in][HROWB], [8 waves][HPART])
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int tile = blockIdx.x, tile_step = gridDim.x, tile_end = a.n_tiles;      // the split kernel's tile order: one contiguous range per XCD
  if (a.xcd) {
    const int per = (a.n_tiles + 7) >> 3, xcd = blockIdx.x & 7;
    tile = xcd * per + (blockIdx.x >> 3);
    tile_step = gridDim.x >> 3;
    tile_end = min(a.n_tiles, (xcd + 1) * per);
  }
  if (tile >= tile_end) return;
  const int kt = a.c_in >> 5, n_pass = a.hidden / TS_QN_HEAD_HIDDEN_STEP;
  const int kg = lane >> 4, q4 = (lane >> 2) & 3, p4 = lane & 3, fr = lane & 15;
  auto key = [](int c) { return ((c & 3) * 5) ^ (((c >> 3) & 1) << 1); };
  // transposed reads (the split kernel's consumer form): lane group kg reads channels 8 kg + q4 (+ 4) of the k-step, frames 16 mt + 4 p4 ..
  int bbase[HMT];
#pragma unroll
  for (int mt = 0; mt < HMT; ++mt) {
    const int c = 8 * kg + q4, t = 16 * mt + 4 * p4;
    bbase[mt] = c * HROWB + (((t >> 3) ^ key(c)) << 4) + ((t & 7) << 1);
  }
  auto read_b = [&](const char* src, int mt) __attribute__((always_inline)) {
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((TS_LDS s16x4*)((TS_LDS char*)src + bbase[mt]));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((TS_LDS s16x4*)((TS_LDS char*)src + bbase[mt] + 4 * HROWB));
    return s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  };

  constexpr int RSRC_FLAGS = 0x00020000;
  auto rsrc = [](const void* p) { return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, 0x7fffffff, RSRC_FLAGS); };
  // (soff is wave-uniform at every call; the readfirstlane keeps it in a scalar register whatever form the compiler gave its computation)
  auto ld16 = [](__amdgpu_buffer_rsrc_t r, int voff, int soff) {
    return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, __builtin_amdgcn_readfirstlane(soff), 0));
  };

  // ---- x tile: a row's 96 frames are 12 sixteen-byte chunks.  Chunks 0..7: thread = (row tid >> 3 of 64, chunk tid & 7), c_in / 64 requests;
  // chunks 8..11: thread = (row tid >> 2 of 128, chunk 8 + (tid & 3)), c_in / 128 requests -- every lane of every request is used, and the
  // requests of a phase differ by a wave-uniform offset.  The swizzle key of a row depends on row % 16 only: so do the LDS addresses.
  // (the addresses are formed where they are used, twice per tile, from a thread index the optimiser cannot trace: kept across the k-loop they
  // would be five more registers in a wave that has none to spare)
  auto opaque = [](int v) { asm volatile("" : "+v"(v)); return v; };
  u32x4 xr[HNX];
  auto x_issue = [&](int tl) __attribute__((always_inline)) {
    const int td = opaque(tid);
    const int rowa = td >> 3, cha = td & 7, rowb = td >> 2, chb = 8 + (td & 3);
    const int xva = (rowa * a.pitch_in + 8 * cha) * 2, xvb = (rowb * a.pitch_in + 8 * chb) * 2;
    const int b = tl / a.n_tt, t0 = (tl - b * a.n_tt) * HT;
    const __amdgpu_buffer_rsrc_t rx = rsrc(a.x + (size_t)b * a.c_in * a.pitch_in + t0);
#pragma unroll
    for (int j = 0; j < 8; ++j) {      // (every call defines every register: nothing of the last tile stays live)
      xr[j] = u32x4{0u, 0u, 0u, 0u};
      if (64 * j < a.c_in) xr[j] = ld16(rx, xva, j * 128 * a.pitch_in);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      xr[8 + j] = u32x4{0u, 0u, 0u, 0u};
      if (128 * j + rowb < a.c_in) xr[8 + j] = ld16(rx, xvb, j * 256 * a.pitch_in);
    }
  };
  auto x_write = [&]() __attribute__((always_inline)) {
    const int td = opaque(tid);
    const int rowa = td >> 3, cha = td & 7, rowb = td >> 2, chb = 8 + (td & 3);
    const int xla = rowa * HROWB + ((cha ^ key(rowa)) << 4), xlb = rowb * HROWB + ((chb ^ key(rowb)) << 4);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (64 * j < a.c_in) *reinterpret_cast<u32x4*>(smem + xla + j * 64 * HROWB) = xr[j];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (128 * j + rowb < a.c_in) *reinterpret_cast<u32x4*>(smem + xlb + j * 128 * HROWB) = xr[8 + j];
  };

  // ---- weight stream: fragment (16-channel tile c16, k-step ks) at byte ((c16 kt + ks) 64 + lane) 16 of w17; the same for every tile, so the
  // stream cycles over (pass, ks) and simply runs on: what it fetches beyond the last tile's last k-step is the first pass again, never used.
  // The ring's slot of a k-step is static: a pass counts kp = round_up(kt, 3) slots, of which those from kt on are skipped by the products
  // (c_in = 512: 16 k-steps in 18 slots -- the first k-step of a pass is requested one real k-step ahead, the others three).
  const __amdgpu_buffer_rsrc_t rw = rsrc(a.w17), rwd = rsrc(a.wd);
  const int lane16 = lane * 16;
  const int kp = (kt + HRING - 1) / HRING * HRING;
  int w_pass = 0, w_ks = 0;                                                // the slot the next ring load fills
  s16x8 ring[HRING][HNT];
  auto w_load = [&](auto sc) __attribute__((always_inline)) {
    constexpr int slot = decltype(sc)::value;
    // (a skipped slot requests the pass's last k-step again: a request under a branch would leave the compiler's wait counts unknown at the
    // top of the k-loop, and it would then drain the ring there)
    const int wk = min(w_ks, kt - 1);
#pragma unroll
    for (int nt = 0; nt < HNT; ++nt)
      ring[slot][nt] = __builtin_bit_cast(s16x8, ld16(rw, lane16, ((((w_pass * HWAVES + wave) * HNT + nt) * kt + wk) << 10)));
    if (++w_ks == kp) {
      w_ks = 0;
      if (++w_pass == n_pass) w_pass = 0;
    }
  };

  f32x4 acc[HMT][HNT];                                                     // hT: (channels 16 nt + 4 kg + i, frame 16 mt + fr)
  f32x4 lacc[HMT][2];                                                      // logitsT: (classes 16 vt + 4 kg + i, frame 16 mt + fr)
  s16x8 wdf[2][2];
  int b = 0, t0 = 0, len_b = 0, pass = 0;

  // the first layer's shift waits in LDS behind the x tile: read from memory at the start of a pass it would be the youngest request in the
  // queue, and the pass's first product would wait for the whole weight ring to land in front of it
  const float* const shift = reinterpret_cast<const float*>(smem + a.lds_main);
  for (int i = tid; i < a.hidden / 4; i += 64 * HWAVES)
    reinterpret_cast<f32x4*>(smem + a.lds_main)[i] = reinterpret_cast<const f32x4*>(a.b17)[i];      // (visible behind the first tile's barrier)
  auto begin_pass = [&]() __attribute__((always_inline)) {
    const int c0 = (pass * HWAVES + wave) * (16 * HNT) + 4 * kg;
#pragma unroll
    for (int nt = 0; nt < HNT; ++nt) {
      const f32x4 bv = *reinterpret_cast<const f32x4*>(shift + c0 + 16 * nt);
#pragma unroll
      for (int mt = 0; mt < HMT; ++mt) acc[mt][nt] = bv;
    }
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int vt = 0; vt < 2; ++vt)
        wdf[p][vt] = __builtin_bit_cast(s16x8, ld16(rwd, lane16, ((((pass * HWAVES + wave) * 2 + p) * 2 + vt) << 10)));
  };
  auto begin_tile = [&]() __attribute__((always_inline)) {                                                // the tile's rows are in xr (requested a tile ago, or in the prologue)
    b = tile / a.n_tt;
    t0 = (tile - b * a.n_tt) * HT;
    len_b = a.len ? min(max(a.len[b], 0), a.t_out) : a.t_out;
    x_write();
    __syncthreads();
#pragma unroll
    for (int vt = 0; vt < 2; ++vt) {
      f32x4 bv = f32x4{0.f, 0.f, 0.f, 0.f};
      if (wave == 0) {
        const int kgo = opaque(lane) >> 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int v = 16 * vt + 4 * kgo + i;
          bv[i] = v < a.n_classes ? a.bd[v] : 0.f;
        }
      }
#pragma unroll
      for (int mt = 0; mt < HMT; ++mt) lacc[mt][vt] = bv;
    }
  };
  // h of this pass, as B fragments, times the decoder's fragments
  auto gemm2 = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int mt = 0; mt < HMT; ++mt) {
      const bool valid = t0 + 16 * mt + fr < len_b;
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        u32x4 hv;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const f32x4 v = acc[mt][2 * p + h];
          hv[2 * h] = valid ? relu_bf16x2(pack_bf16(v[0], v[1])) : 0u;
          hv[2 * h + 1] = valid ? relu_bf16x2(pack_bf16(v[2], v[3])) : 0u;
        }
        const s16x8 hf = __builtin_bit_cast(s16x8, hv);
#pragma unroll
        for (int vt = 0; vt < 2; ++vt) lacc[mt][vt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wdf[p][vt], hf, lacc[mt][vt], 0, 0, 0);
      }
    }
  };
  auto end_tile = [&]() __attribute__((always_inline)) {
    const int next = tile + tile_step;
    x_issue(next < tile_end ? next : tile);                                // in flight through the reduction (after the last tile: its own rows again, unused)
    __syncthreads();                                                       // every wave is done with the x tile
    f32x4* const all = reinterpret_cast<f32x4*>(smem);
    f32x4* const mine = all + wave * (HPART / 16);
#pragma unroll
    for (int mt = 0; mt < HMT; ++mt)
#pragma unroll
      for (int vt = 0; vt < 2; ++vt) mine[(mt * 2 + vt) * 64 + lane] = lacc[mt][vt];
    __syncthreads();
    if (wave < HMT) {                                                      // wave w finishes frames [16 w, 16 w + 16) of the tile
      const int ln = opaque(lane), kgo = ln >> 4;
      const int t = t0 + 16 * wave + (ln & 15);
#pragma unroll
      for (int vt = 0; vt < 2; ++vt) {
        f32x4 s = all[(wave * 2 + vt) * 64 + lane];
#pragma unroll
        for (int w = 1; w < HWAVES; ++w) s += all[w * (HPART / 16) + (wave * 2 + vt) * 64 + lane];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int v = 16 * vt + 4 * kgo + i;
          if (v < a.n_classes && t < a.t_out) a.y[((size_t)b * a.n_classes + v) * a.pitch_out + t] = s[i];
        }
      }
    }
    __syncthreads();                                                       // the sums are read: the next tile's rows may land
    tile = next;
  };
  // one k-step: 6 x 4 products; the x fragments stream through three registers (the one being multiplied and two in flight from LDS)
  auto kstep = [&](auto sc, int ks) __attribute__((always_inline)) {
    constexpr int slot = decltype(sc)::value;
    if (ks < kt) {
      const char* const src = smem + ks * (32 * HROWB);
      s16x8 bf[3];
      bf[0] = read_b(src, 0);
      bf[1] = read_b(src, 1);
#pragma unroll
      for (int mt = 0; mt < HMT; ++mt) {
        if (mt + 2 < HMT) bf[(mt + 2) % 3] = read_b(src, mt + 2);
#pragma unroll
        for (int nt = 0; nt < HNT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ring[slot][nt], bf[mt % 3], acc[mt][nt], 0, 0, 0);
      }
      // the order above is the order wanted: two x fragments in flight from LDS under every four products
      __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
#pragma unroll
      for (int mt = 0; mt < HMT; ++mt) {
        if (mt + 2 < HMT) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, HNT, 0);
      }
    }
    w_load(sc);                                                            // the slot just used takes the one three ahead
  };

  x_issue(tile);
  static_for<0, HRING>([&](auto sc) { w_load(sc); });
  while (tile < tile_end) {
    begin_tile();
    for (pass = 0; pass < n_pass; ++pass) {
      begin_pass();
      for (int ks = 0; ks < kt; ks += HRING) static_for<0, HRING>([&](auto sc) { kstep(sc, ks + decltype(sc)::value); });
      gemm2();
    }
    end_tile();
  }
}

std::atomic<long long> head_launches{0};

}  // namespace

}  // namespace ts

extern "C" {

int ts_qn_head_abi_version(void) { return TS_QN_HEAD_ABI_VERSION; }

int64_t ts_qn_head_launches(void) { return (int64_t)ts::head_launches.load(); }

int ts_qn_head_fwd(const void* x, const int32_t* len_out, const void* w17, const float* b17, const void* wd, const float* bd, float* logits,
                   int32_t batch, int32_t c_in, int32_t hidden, int32_t n_classes, int32_t t_out, int32_t pitch_in, int32_t pitch_out,
                   int32_t kernel, int32_t stride, int32_t c_res, void* stream_) {
  using namespace ts;
  if (!x || !w17 || !b17 || !wd || !bd || !logits || batch <= 0 || c_in <= 0 || hidden <= 0 || n_classes <= 0 || t_out <= 0) return TS_EINVAL;
  if (n_classes > TS_QN_HEAD_V_MAX || c_in % 64 || c_in > TS_QN_HEAD_CIN_MAX || hidden % TS_QN_HEAD_HIDDEN_STEP || hidden > TS_QN_HEAD_HIDDEN_MAX)
    return TS_EUNSUPPORTED;
  if (kernel != 1 || stride != 1 || c_res != 0) return TS_EUNSUPPORTED;
  const long long n_tt = ((long long)t_out + HT - 1) / HT;
  if (pitch_in % 8 || pitch_in < n_tt * HT || pitch_out < t_out) return TS_EUNSUPPORTED;
  if (misaligned(x) || misaligned(w17) || misaligned(wd) || misaligned(b17) || misaligned(bd, 3) || misaligned(logits, 3) || misaligned(len_out, 3))
    return TS_EUNSUPPORTED;
  // tiles are counted and a clip's rows are addressed in 32 bits (byte offsets from the clip's first row)
  if (n_tt * batch > 0x7fffffffll || 2ll * c_in * pitch_in > 0x7fffffffll) return TS_EUNSUPPORTED;
  TS_STREAM;
  HeadArgs a{static_cast<const unsigned short*>(x), len_out, static_cast<const unsigned short*>(w17), b17, static_cast<const unsigned short*>(wd), bd,
             logits, batch, c_in, hidden, n_classes, t_out, pitch_in, pitch_out, (int)n_tt, (int)(n_tt * batch), 0, 0};
  a.lds_main = c_in * HROWB > HWAVES * HPART ? c_in * HROWB : HWAVES * HPART;      // the x tile, then the eight partial sums
  const size_t lds = (size_t)a.lds_main + (size_t)hidden * 4;                     // + the shift
  static bool attr_set[64] = {};                          // per device (one process may drive several GPUs)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return TS_EINVAL;
  if (!attr_set[dev]) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(qn_head_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return (int)e;
    attr_set[dev] = true;
  }
  const int n_cu = cu_count();
  const int grid = a.n_tiles < n_cu ? a.n_tiles : n_cu;
  a.xcd = grid % 8 == 0 ? 1 : 0;
  (void)hipGetLastError();
  hipLaunchKernelGGL(qn_head_kernel, dim3((unsigned)grid), dim3(64 * HWAVES), lds, stream, a);
  const int st = hip_status(hipGetLastError());
  if (st == TS_OK) head_launches.fetch_add(1);
  return st;
}

}  // extern "C"
