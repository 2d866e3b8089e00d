// CTC forced alignment for transcripts beyond ts_ctc_align's 2 047 labels (a lecture, an audiobook chapter), for gfx950.
// No reference counterpart.  ABI: include_open/thunder_speech_amd/longform.h.
//
// ts_ctc_align_long is ts_ctc_align (csrc/ctc_align.hip) in another layout; inputs, outputs, tie rules and arithmetic are that kernel's, the path's
// log-probabilities and the whole epilogue are shared text (ctc_align_common.hpp).  What differs, and why:
//   * still ONE workgroup per utterance and no waiting across workgroups: the recursion is a chain of T steps whose step needs every state of the
//     step before, and a workgroup that spins on another's flag can hang a machine that others share.  So the states a workgroup can hold bound the
//     transcript: each thread owns SPT = 8 .. 64 CONTIGUOUS states in registers (state s = tid * SPT + i) where ts_ctc_align gives thread `lane`
//     the states lane + i * NT through two LDS rows;
//   * a thread updates its block in place from the high state down, so a[i - 1] and a[i - 2] are still the previous frame's when a[i] is formed.
//     Only state 0 of a block looks outside it, at the neighbour's highest state (SPT is even, a block starts on a blank state, and a blank state
//     is never skipped into; the block's state 1 is skipped into from that same cell): ONE float per thread and frame crosses through LDS, double
//     buffered, behind one LDS-ordering barrier;
//   * the emissions: a frame's V logits are staged in LDS once, as one contiguous row, and every state reads its token's cell there (a thread's
//     32 label states would otherwise hold 32 global loads in flight per frame).  The ring holds 2 LONG_PF frames: step k requests frame
//     k + LONG_PF and writes to LDS what step k - 1 requested, so no step waits for a load of its own;
//   * the back-pointers, 2 bits per state (0 stay, 1 from s - 1, 2 from s - 2), always go to the workspace: one store of 2 SPT bits per thread and
//     frame into a row that is a flat array of 2-bit codes (state s: bits 2 (s & 15) of 32-bit word s >> 4), whatever SPT;
//   * the backtrace fetches 16 frames per round trip as ts_ctc_align's does: 16 frames back the path is at most 30 states down, in word s >> 4 or
//     one of the two below; 64 lanes fetch 16 frames x 4 words.
#include "ctc_align_common.hpp"

#include "thunder_speech_amd/longform.h"

namespace ts {

constexpr int LONG_PF = 8;                           // emission prefetch distance in time steps (ALIGN_PF of csrc/ctc_align.hip)
constexpr int LONG_RING = 2 * LONG_PF;               // frames in the LDS emission ring
constexpr int LONG_TH_MAX = 1024;
constexpr size_t LONG_LDS_MAX = 160 * 1024;

struct AlignLongArgs {
  const float* logits;      // [B][V][pitch]
  const int* targets;       // [B][s_max]
  const int* input_len;
  const int* target_len;
  int* path;                // [B][n_frames]
  int* spans;               // [B][s_max][2]
  float* span_logp;         // [B][s_max]
  float* score;             // [B]
  unsigned* bp;             // workspace [B][n_frames][row_words]
  int* state;               // workspace [B][n_frames]   the path's state per frame
  float* lp;                // workspace [B][n_frames]   the path's log-probability per frame
  int n_classes, n_frames, pitch, s_max, blank;
  int row_words;            // 32-bit words per back-pointer row: round_up(2 s_max + 1, 64) / 16
};

template <int SPT>
__global__ __launch_bounds__(LONG_TH_MAX) void ctc_align_long_kernel(const AlignLongArgs a) {
  static_assert(SPT % 16 == 0 || SPT == 8, "a thread's back-pointers are whole 32-bit words, or one 16-bit half");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int V = a.n_classes, NT = blockDim.x;
  float* const ring = reinterpret_cast<float*>(smem);            // [LONG_RING][V]: row k % LONG_RING holds the logits of frame k
  float* const xch = ring + (size_t)LONG_RING * V;             // [2][NT + 1]: cell tid + 1 is thread tid's highest state; cell 0 stays -inf
  float* const red = xch + 2 * (NT + 1);                         // [16]
  float* const fin = red + 16;                                   // [2]: the last two states after the last frame
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int T = a.input_len[b];
  T = T < 0 ? 0 : (T > a.n_frames ? a.n_frames : T);
  int S = a.target_len[b];
  S = S < 0 ? 0 : (S > a.s_max ? a.s_max : S);
  const int L = 2 * S + 1, blank = a.blank;
  const float* lg = a.logits + (size_t)b * V * a.pitch;
  const int* const tg = a.targets + (size_t)b * a.s_max;
  unsigned* const bp = a.bp + (size_t)b * a.n_frames * a.row_words;
  int* const st = a.state + (size_t)b * a.n_frames;
  float* const lpw = a.lp + (size_t)b * a.n_frames;
  int* const path = a.path + (size_t)b * a.n_frames;
  int* const spans = a.spans + (size_t)b * a.s_max * 2;
  float* const span_logp = a.span_logp + (size_t)b * a.s_max;
  auto label = [&](int j) { return min(max(tg[j], 0), V - 1); };          // an id outside [0, V) is read as the nearest valid one
  auto token = [&](int s) { return (s & 1) ? label(s >> 1) : blank; };

  // my block: states base .. base + SPT; the odd ones are label states (label base / 2 + i), `skip` bit i: label state i may be entered from two below
  const int base = tid * SPT;
  // two label states per register: in each 16-bit half the class id (n_classes <= TS_CTC_ALIGN_LONG_V_MAX < 2^15) and, in bit 15, whether the state
  // may be entered from two below (its label differs from the one before); label i in half i & 1 of tok2[i >> 1]
  unsigned tok2[SPT / 4] = {};
  int before = (base >= 2 && base / 2 - 1 < S) ? label(base / 2 - 1) : -1;       // the label below my first one
#pragma unroll
  for (int i = 0; i < SPT / 2; ++i) {
    const int j = base / 2 + i;
    const bool act = j < S;
    const int tk = act ? label(j) : blank;             // states at or beyond L never feed a state below them: they need no guard, only a valid cell
    const bool skip = act && j >= 1 && tk != before;
    tok2[i >> 1] |= ((unsigned)tk | (skip ? 0x8000u : 0u)) << (16 * (i & 1));
    before = tk;
    if (i & 1) asm volatile("" : "+v"(tok2[i >> 1]));                             // packed here, not sunk to where 32 ids and 32 conditions are live
  }
  auto half = [&](int i) { return (tok2[i >> 1] >> (16 * (i & 1))) & 0xFFFFu; };
  auto tok = [&](int i) { return (int)(half(i) & 0x7FFFu); };
  float al[SPT];
#pragma unroll
  for (int i = 0; i < SPT; ++i) al[i] = ALIGN_NEG_INF;
  // "frame -1": the path starts in state 0 or 1, which is what the recursion makes of a single finite state 0 (0 + x is x, bit for bit).  Frame 0
  // then is a step like every other; its back-pointer row is written and never read
  if (tid == 0) al[0] = 0.f;

  // the emission ring: row k & 15 holds frame k's V logits.  Step k requests frame k + LONG_PF into registers and writes what step k - 1 requested:
  // a frame is in LDS seven steps before its use, in a row last read eight steps ago.  Frames at or beyond T are read as frame T - 1 (logits at
  // t >= T are not read) and never consumed
  auto row_of = [&](int k) { return ring + (size_t)(k & (LONG_RING - 1)) * V; };
  constexpr int LONG_SR = SPT == 64 ? 1 : 2;           // staged logits per thread and step that wait in registers for one step (64 states leave room for one)
  float sreg[LONG_SR];
  // the first LONG_SR classes per thread wait in registers until the next step; the rest (V > LONG_SR NT: a large vocabulary under a small
  // workgroup) are written at once
  auto stage_load = [&](int k) {
    const int t = min(k, T - 1);
#pragma unroll
    for (int r = 0; r < LONG_SR; ++r) sreg[r] = lg[(size_t)min(tid + r * NT, V - 1) * a.pitch + t];
#pragma clang loop vectorize(disable) unroll(disable)
    for (int i = tid + LONG_SR * NT; i < V; i += NT) row_of(k)[i] = lg[(size_t)i * a.pitch + t];
  };
  auto stage_store = [&](int k) {
#pragma unroll
    for (int r = 0; r < LONG_SR; ++r)
      if (tid + r * NT < V) row_of(k)[tid + r * NT] = sreg[r];
  };

  for (int i = tid; i < 2 * (NT + 1); i += NT) xch[i] = ALIGN_NEG_INF;
  if (T > 0)
    for (int k = 0; k < LONG_PF; ++k)                                      // frames 0 .. LONG_PF - 1, before the first step
      for (int i = tid; i < V; i += NT) row_of(k)[i] = lg[(size_t)i * a.pitch + min(k, T - 1)];
  __syncthreads();

  for (int k = 0; k < T; ++k) {
    {
      if (k > 0) stage_store(k - 1 + LONG_PF);
      stage_load(k + LONG_PF);
      const float* const row = row_of(k);
      const float* const xr = xch + ((k & 1) ? 0 : NT + 1);               // written in step k - 1
      float* const xw = xch + ((k & 1) ? NT + 1 : 0);
      {
        const float n1 = xr[tid];                      // state base - 1 in the previous frame
        // the ids are opaque to the optimiser from here: hoisted out of the frame loop, the states' LDS addresses and skip conditions would
        // outlive every frame in registers that the 64-state block has no room for
#pragma unroll
        for (int q = 0; q < SPT / 4; ++q) asm volatile("" : "+v"(tok2[q]));
        const float eb = row[blank];
        unsigned code[(SPT + 15) / 16] = {};
#pragma unroll
        for (int i = SPT - 1; i >= 0; --i) {           // high to low: al[i - 1] and al[i - 2] are still the previous frame's
          // the tie rule: stay beats s-1, s-1 beats s-2 (ts_ctc_align's strict comparisons in that order, as equalities with the maximum)
          const float own = al[i], p1 = i >= 1 ? al[i - 1] : n1;
          float best = fmaxf(own, p1), e = eb;
          if (i & 1) {
            const float p2 = i >= 2 ? al[i - 2] : n1;
            best = fmaxf(best, (half(i >> 1) & 0x8000u) ? p2 : ALIGN_NEG_INF);
            e = row[tok(i >> 1)];
          }
          const unsigned cd = best == own ? 0u : (best == p1 ? 1u : 2u);
          al[i] = best + e;
          code[i >> 4] |= cd << (2 * (i & 15));
          // the SPT updates of a frame are independent, and ordered freely their emissions, maxima and codes are all live at once, next to the old
          // and the new values: eight states at a time, finished (opaque to the optimiser) before the next eight begin
          if (i % 8 == 0) {
#pragma unroll
            for (int u = 0; u < 8; ++u) asm volatile("" : "+v"(al[i + u]));
            asm volatile("" : "+v"(code[i >> 4]));
          }
        }
        if (base < L) {                                // the row holds round_up(L, 64) states: every block that starts below L ends inside it
          unsigned* const at = bp + (size_t)k * a.row_words;
          if constexpr (SPT == 8) reinterpret_cast<unsigned short*>(at)[tid] = (unsigned short)code[0];
          else if constexpr (SPT == 16) at[tid] = code[0];
          else if constexpr (SPT == 32) reinterpret_cast<uint2*>(at)[tid] = uint2{code[0], code[1]};
          else reinterpret_cast<uint4*>(at)[tid] = uint4{code[0], code[1], code[2], code[3]};
        }
      }
      xw[tid + 1] = al[SPT - 1];
      align_lds_barrier();
    }
  }
  // where the path ends: the last label state unless the final blank is strictly better
#pragma unroll
  for (int i = 0; i < SPT; ++i) {
    if (base + i == L - 1) fin[0] = al[i];
    if (base + i == L - 2) fin[1] = al[i];
  }
  __syncthreads();                                     // and the back-pointers in the workspace are visible to wave 0
  bool feasible;
  int s_end = 0;
  if (T == 0) {
    feasible = S == 0;
  } else {
    const float fb = fin[0], fl = L > 1 ? fin[1] : ALIGN_NEG_INF;
    s_end = (L > 1 && !(fb > fl)) ? L - 2 : L - 1;
    feasible = fmaxf(fb, fl) > ALIGN_NEG_INF;
  }
  if (wave == 0 && feasible && T > 0) {                // the backtrace: one wave, every lane with the same state
    int s = s_end, t = T - 1;
    while (t >= 1) {
      // lane = (frame, word): frames t .. t - 15, words s >> 4 .. (s >> 4) - 3
      const int hi = s >> 4;
      const unsigned w = bp[(size_t)max(t - (lane >> 2), 0) * a.row_words + max(hi - (lane & 3), 0)];
      const int n = min(16, t);                        // frames t, t-1, ..., t-n+1: all >= 1 (frame 0 has no back-pointers)
      for (int j = 0; j < n; ++j) {
        if (lane == 0) st[t - j] = s;
        const unsigned ws = __shfl(w, j * 4 + min(hi - (s >> 4), 3));
        s = max(s - (int)((ws >> (2 * (s & 15))) & 3u), 0);
      }
      t -= n;
    }
    if (lane == 0) st[0] = s;
  }
  __syncthreads();
  align_epilogue(lg, V, a.pitch, a.n_frames, a.s_max, T, S, L, feasible, st, lpw, path, spans, span_logp, a.score + b, red, token);
}

}  // namespace ts

// What ts_ctc_align_long launches; ts_ctc_align_long launches from this and ts_ctc_align_long_launch_config reports it.
struct AlignLongLaunch {
  int spt, threads, which;
  size_t lds;
};
static int align_long_launch_config(int n_frames, int s_max, int spt_in, int n_classes, AlignLongLaunch* c) {
  if (n_frames <= 0 || s_max < 0 || n_classes <= 0) return TS_EINVAL;
  if (spt_in != 0 && spt_in != 8 && spt_in != 16 && spt_in != 32 && spt_in != 64) return TS_EINVAL;
  if (s_max > TS_CTC_ALIGN_LONG_S_MAX || n_classes > TS_CTC_ALIGN_LONG_V_MAX) return TS_EUNSUPPORTED;
  const int lmax = 2 * s_max + 1;
  int spt = spt_in;
  if (spt == 0)
    for (spt = 8; lmax > spt * ts::LONG_TH_MAX; spt *= 2) {}
  if (lmax > spt * ts::LONG_TH_MAX) return TS_EINVAL;
  c->spt = spt;
  c->which = spt == 8 ? 0 : (spt == 16 ? 1 : (spt == 32 ? 2 : 3));
  c->threads = ((lmax + spt - 1) / spt + 63) / 64 * 64;
  c->lds = ((size_t)ts::LONG_RING * n_classes + 2 * (c->threads + 1) + 16 + 4) * sizeof(float);
  return c->lds <= ts::LONG_LDS_MAX ? TS_OK : TS_EUNSUPPORTED;
}
static int align_long_row_words(int s_max) { return (2 * s_max + 1 + 63) / 64 * 4; }

extern "C" int ts_ctc_align_long_launch_config(int32_t n_frames, int32_t s_max, int32_t states_per_thread_in, int32_t n_classes,
                                               int32_t* states_per_thread, int32_t* threads, int32_t* lds_bytes) {
  if (!states_per_thread || !threads || !lds_bytes) return TS_EINVAL;
  AlignLongLaunch c{};
  const int st = align_long_launch_config(n_frames, s_max, states_per_thread_in, n_classes, &c);
  if (st != TS_OK) return st;
  *states_per_thread = c.spt; *threads = c.threads; *lds_bytes = (int32_t)c.lds;
  return TS_OK;
}

extern "C" int64_t ts_ctc_align_long_workspace_bytes(int32_t batch, int32_t n_frames, int32_t s_max) {
  if (batch <= 0 || n_frames <= 0 || s_max < 0) return TS_EINVAL;
  if (s_max > TS_CTC_ALIGN_LONG_S_MAX) return TS_EUNSUPPORTED;
  return (int64_t)batch * n_frames * ((int64_t)align_long_row_words(s_max) * (int64_t)sizeof(unsigned) + (int64_t)(sizeof(int) + sizeof(float)));
}

extern "C" int ts_ctc_align_long(const float* logits, int32_t batch, int32_t n_classes, int32_t n_frames, int32_t pitch, const int32_t* targets,
                                 int32_t s_max, const int32_t* input_len, const int32_t* target_len, int32_t blank, int32_t states_per_thread,
                                 int32_t* path, int32_t* spans, float* span_logp, float* score, void* workspace, void* stream_) {
  using namespace ts;
  if (!logits || !targets || !input_len || !target_len || !path || !spans || !span_logp || !score || !workspace) return TS_EINVAL;
  if (batch <= 0 || n_classes <= 0 || n_frames <= 0 || pitch < n_frames || s_max < 0) return TS_EINVAL;
  if (blank < 0 || blank >= n_classes) return TS_EINVAL;
  AlignLongLaunch cfg{};
  const int cst = align_long_launch_config(n_frames, s_max, states_per_thread, n_classes, &cfg);
  if (cst != TS_OK) return cst;
  if (misaligned(workspace)) return TS_EUNSUPPORTED;
  TS_STREAM;
  AlignLongArgs a{};
  a.logits = logits; a.targets = targets; a.input_len = input_len; a.target_len = target_len;
  a.path = path; a.spans = spans; a.span_logp = span_logp; a.score = score;
  a.n_classes = n_classes; a.n_frames = n_frames; a.pitch = pitch; a.s_max = s_max; a.blank = blank;
  a.row_words = align_long_row_words(s_max);
  char* ws = static_cast<char*>(workspace);
  a.bp = reinterpret_cast<unsigned*>(ws);
  ws += (size_t)batch * n_frames * a.row_words * sizeof(unsigned);
  a.state = reinterpret_cast<int*>(ws);
  a.lp = reinterpret_cast<float*>(ws + (size_t)batch * n_frames * sizeof(int));
  const void* const fns[4] = {reinterpret_cast<const void*>(ctc_align_long_kernel<8>), reinterpret_cast<const void*>(ctc_align_long_kernel<16>),
                              reinterpret_cast<const void*>(ctc_align_long_kernel<32>), reinterpret_cast<const void*>(ctc_align_long_kernel<64>)};
  const void* const fn = fns[cfg.which];
  static bool big_all[64][4] = {};                     // more than the default 64 KiB allowed: per (device, instantiation)
  if (cfg.lds > 64 * 1024) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return TS_EINVAL;
    if (!big_all[dev][cfg.which]) {
      if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LONG_LDS_MAX) != hipSuccess) return TS_EUNSUPPORTED;
      big_all[dev][cfg.which] = true;
    }
  }
  void* params[] = {&a};
  const hipError_t e = hipLaunchKernel(fn, dim3(batch), dim3((unsigned)cfg.threads), params, cfg.lds, stream);
  if (e != hipSuccess) return (int)e;
  return hip_status(hipGetLastError());
}
