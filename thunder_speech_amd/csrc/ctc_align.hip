// CTC forced alignment (Viterbi over the blank-extended target) and the frame spans of the greedy transcript, for gfx950.
// No reference counterpart: the reference returns bare strings (module.py:98-101).  ABI: include/thunder_speech_amd/ctc_align.h.
//
// ts_ctc_align keeps the skeleton of csrc/ctc.hip's alpha recursion -- one workgroup per utterance, the L = 2S+1 states spread over the lanes
// (1, 2 or 4 per thread), two LDS rows with -inf guard cells, the emissions requested a chunk of frames ahead, a barrier per step that orders
// LDS traffic only -- with max in place of log-sum-exp.  Three things differ:
//   * the serial chain runs on the RAW logits: every path visits every frame exactly once, so the per-frame log-sum-exp shifts all paths alike and
//     the arg-max path needs no exponential and no logarithm.  The normaliser is computed afterwards, for the T cells of the path only, in
//     parallel over the frames;
//   * each step leaves 2 bits per state, the transition taken (0 stay, 1 from s-1, 2 from s-2), as two wave ballots: 16 bytes per frame and
//     wave-slot, written by one lane.  They live in LDS when the clip fits (BP_LDS: 80 KB at T = 999, S = 150), else in the workspace;
//   * one wave walks the back-pointers from the last frame to the first: a chain of T LDS reads, or, from the workspace, of T / 16 round trips
//     (the path moves at most two states per frame, so 16 frames back it is in the same 64-state word or the one below: 64 lanes fetch
//     16 frames x 2 words x 2 ballots at once).
#include "ctc_align_common.hpp"      // ALIGN_NEG_INF, align_lds_barrier, frame_logp: shared with csrc/ctc_align_long.hip

#include "thunder_speech_amd/ctc_align.h"

namespace ts {

constexpr int ALIGN_PF = 8;                          // emission prefetch distance in time steps
constexpr size_t ALIGN_LDS_MAX = 160 * 1024;
constexpr int ALIGN_RED_BYTES = 64;                  // 16 floats: the score's per-wave partial sums

struct AlignArgs {
  const float* logits;      // [B][V][pitch]
  const int* targets;       // [B][s_max]
  const int* input_len;
  const int* target_len;
  int* path;                // [B][n_frames]
  int* spans;               // [B][s_max][2]
  float* span_logp;         // [B][s_max]
  float* score;             // [B]
  ulonglong2* bp;           // workspace [B][n_frames][nwt]   (the instantiations without BP_LDS)
  int* state;               // workspace [B][n_frames]   the path's state per frame
  float* lp;                // workspace [B][n_frames]   the path's log-probability per frame
  int n_classes, n_frames, pitch, s_max, lmax, blank;
  int nwt;                  // 64-state words per frame: states per thread x waves (state s is bit s & 63 of word s >> 6)
};

template <int SPT, bool BP_LDS>
__global__ __launch_bounds__(1024) void ctc_align_kernel(const AlignArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int L_MAX = a.lmax, NWT = a.nwt, V = a.n_classes;
  ulonglong2* const bp_l = reinterpret_cast<ulonglong2*>(smem);                                      // [n_frames][nwt] (BP_LDS)
  float* const red = reinterpret_cast<float*>(smem + (BP_LDS ? (size_t)a.n_frames * NWT * sizeof(ulonglong2) : 0));   // [16]
  float* const row0 = red + ALIGN_RED_BYTES / sizeof(float);   // [lmax + 4]: two -inf guard cells on either side
  float* const row1 = row0 + L_MAX + 4;
  int* const ext = reinterpret_cast<int*>(row1 + L_MAX + 4);   // [lmax]
  const int b = blockIdx.x, lane = threadIdx.x, wave = threadIdx.x >> 6;
  const int NT = blockDim.x;                                   // round_up(lmax / SPT, 64) threads: state s = lane + i * NT
  int T = a.input_len[b];
  T = T < 0 ? 0 : (T > a.n_frames ? a.n_frames : T);
  int S = a.target_len[b];
  S = S < 0 ? 0 : (S > a.s_max ? a.s_max : S);
  const int L = 2 * S + 1;
  const float* lg = a.logits + (size_t)b * V * a.pitch;
  ulonglong2* const bp_g = BP_LDS ? nullptr : a.bp + (size_t)b * a.n_frames * NWT;
  int* const st = a.state + (size_t)b * a.n_frames;
  float* const lpw = a.lp + (size_t)b * a.n_frames;
  int* const path = a.path + (size_t)b * a.n_frames;
  int* const spans = a.spans + (size_t)b * a.s_max * 2;
  float* const span_logp = a.span_logp + (size_t)b * a.s_max;

  for (int s = lane; s < L; s += NT) ext[s] = (s & 1) ? min(max(a.targets[(size_t)b * a.s_max + (s >> 1)], 0), V - 1) : a.blank;
  for (int s = lane; s < L_MAX + 4; s += NT) { row0[s] = ALIGN_NEG_INF; row1[s] = ALIGN_NEG_INF; }
  __syncthreads();
  float* prev = row0 + 2;
  float* cur = row1 + 2;

  constexpr int NS = SPT;
  bool act[NS], skip[NS], init[NS];
  const float* lrow[NS];
  float own[NS], pf[2][ALIGN_PF][NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const int s = lane + i * NT;
    act[i] = s < L;
    const int e = act[i] ? ext[s] : a.blank;
    skip[i] = act[i] && s >= 2 && e != a.blank && e != ext[s - 2];   // into a label state from a different label two states below
    init[i] = s < 2 && act[i];
    lrow[i] = lg + (size_t)e * a.pitch;
    own[i] = ALIGN_NEG_INF;
  }
  // emissions are requested a whole chunk of ALIGN_PF steps ahead, for lanes without a state from the blank's row and with clamped frame
  // indices: all loads unconditional, no vector-memory wait inside a chunk (csrc/ctc.hip:57-68)
  auto fetch = [&](float (&buf)[ALIGN_PF][NS], int k0) {
#pragma unroll
    for (int j = 0; j < ALIGN_PF; ++j)
#pragma unroll
      for (int i = 0; i < NS; ++i) buf[j][i] = lrow[i][min(k0 + j, T - 1)];
  };
  auto chunk = [&](float (&buf)[ALIGN_PF][NS], int k0) {
#pragma unroll
    for (int j = 0; j < ALIGN_PF; ++j) {
      const int k = k0 + j;
      if (k < T) {                                 // workgroup-uniform
        float n1[NS], n2[NS];
#pragma unroll
        for (int i = 0; i < NS; ++i) {             // all LDS reads of the step first
          const int s = act[i] ? lane + i * NT : 0;
          n1[i] = prev[s - 1];
          n2[i] = prev[s - 2];
        }
#pragma unroll
        for (int i = 0; i < NS; ++i) {
          // the tie rule: stay beats s-1, s-1 beats s-2 (strict comparisons in that order)
          float best = own[i];
          int code = 0;
          if (n1[i] > best) { best = n1[i]; code = 1; }
          const float n2v = skip[i] ? n2[i] : ALIGN_NEG_INF;
          if (n2v > best) { best = n2v; code = 2; }
          float v = best + buf[j][i];
          if (k == 0) v = init[i] ? buf[j][i] : ALIGN_NEG_INF;
          own[i] = v;
          ulonglong2 w;
          w.x = __ballot(code == 1);
          w.y = __ballot(code == 2);
          if ((lane & 63) == 0) {                  // every wave and slot writes its word at every step: nothing of [0, T) x [0, nwt) stays unwritten
            const size_t at = (size_t)k * NWT + i * (NT >> 6) + wave;
            if constexpr (BP_LDS) bp_l[at] = w; else bp_g[at] = w;
          }
        }
#pragma unroll
        for (int i = 0; i < NS; ++i)
          if (act[i]) cur[lane + i * NT] = own[i];
        align_lds_barrier();
        float* tmp = prev; prev = cur; cur = tmp;
      }
    }
    fetch(buf, k0 + 2 * ALIGN_PF);                 // the chunk after next, into the buffer just used
  };
  if (T > 0) {
    fetch(pf[0], 0);
    fetch(pf[1], ALIGN_PF);
    for (int k0 = 0; k0 < T; k0 += 2 * ALIGN_PF) {
      chunk(pf[0], k0);
      chunk(pf[1], k0 + ALIGN_PF);
    }
  }
  // where the path ends: the last label state unless the final blank is strictly better
  bool feasible;
  int s_end = 0;
  if (T == 0) {
    feasible = S == 0;
  } else {
    const float fb = prev[L - 1], fl = L > 1 ? prev[L - 2] : ALIGN_NEG_INF;
    s_end = (L > 1 && !(fb > fl)) ? L - 2 : L - 1;
    feasible = fmaxf(fb, fl) > ALIGN_NEG_INF;
  }
  __syncthreads();                                 // the back-pointers in the workspace are visible to wave 0
  if (wave == 0 && feasible && T > 0) {            // the backtrace: one wave, every lane with the same state
    int s = s_end;
    if constexpr (BP_LDS) {
      for (int t = T - 1; t >= 1; --t) {
        if (lane == 0) st[t] = s;
        const ulonglong2 w = bp_l[(size_t)t * NWT + (s >> 6)];
        const int sh = s & 63;
        s = max(s - ((int)((w.x >> sh) & 1ull) + 2 * (int)((w.y >> sh) & 1ull)), 0);
      }
    } else {
      const unsigned long long* const words = reinterpret_cast<const unsigned long long*>(bp_g);
      int t = T - 1;
      while (t >= 1) {
        // 16 frames back the path is in word s >> 6 or in the one below: lane = (frame, word, ballot)
        const int hi = s >> 6, lo = hi > 0 ? hi - 1 : 0;
        const int f = max(t - (lane >> 2), 0);
        const unsigned long long w = words[((size_t)f * NWT + ((lane & 2) ? lo : hi)) * 2 + (lane & 1)];
        const int n = min(16, t);                  // frames t, t-1, ..., t-n+1: all >= 1
        for (int j = 0; j < n; ++j) {
          if (lane == 0) st[t - j] = s;
          const int src = j * 4 + ((s >> 6) == hi ? 0 : 2);
          const unsigned long long w0 = __shfl(w, src), w1 = __shfl(w, src + 1);
          const int sh = s & 63;
          s = max(s - ((int)((w0 >> sh) & 1ull) + 2 * (int)((w1 >> sh) & 1ull)), 0);
        }
        t -= n;
      }
    }
    if (lane == 0) st[0] = s;
  }
  __syncthreads();
  align_epilogue(lg, V, a.pitch, a.n_frames, a.s_max, T, S, L, feasible, st, lpw, path, spans, span_logp, a.score + b, red, [&](int s) { return ext[s]; });
}

// Greedy spans, one 1024-thread workgroup per utterance.  Pass 1, a thread per frame: argmax (lowest index wins, as greedy_kernel of
// csrc/decode.hip) and that class's log-probability, into the workspace.  Pass 2, in chunks of 1024 frames: run heads by comparison with the
// frame before, a prefix count of the heads that are not blank (ballot, per-wave totals, a running carry), and the head's thread follows its
// run to its end, 8 independent loads at a time, summing in frame order.
constexpr int GSP_TH = 1024, GSP_W = GSP_TH / 64;
__global__ __launch_bounds__(GSP_TH) void ctc_greedy_spans_kernel(const float* __restrict__ logits, int n_classes, int n_frames, int pitch,
                                                                  const int* __restrict__ input_len, int blank, int* __restrict__ tokens,
                                                                  int* __restrict__ spans, float* __restrict__ span_logp, int* __restrict__ counts,
                                                                  int* ids_ws, float* lp_ws) {
  __shared__ int wave_total[GSP_W];
  __shared__ int carry_s;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* lg = logits + (size_t)b * n_classes * pitch;
  int T = input_len ? input_len[b] : n_frames;
  T = T < 0 ? 0 : (T > n_frames ? n_frames : T);
  int* const ids = ids_ws + (size_t)b * n_frames;
  float* const lps = lp_ws + (size_t)b * n_frames;
  int* const tok_o = tokens + (size_t)b * n_frames;
  int* const span_o = spans + (size_t)b * n_frames * 2;
  float* const logp_o = span_logp + (size_t)b * n_frames;
  if (tid == 0) carry_s = 0;
  for (int t = tid; t < T; t += GSP_TH) {
    float bv = lg[t];
    int best = 0;
    for (int v0 = 1; v0 < n_classes; v0 += 8) {
      float x[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) x[u] = lg[(size_t)min(v0 + u, n_classes - 1) * pitch + t];
#pragma unroll
      for (int u = 0; u < 8; ++u) if (v0 + u < n_classes && x[u] > bv) { bv = x[u]; best = v0 + u; }
    }
    ids[t] = best;
    lps[t] = frame_logp(lg, n_classes, pitch, t, best);
  }
  __syncthreads();
  for (int t0 = 0; t0 < T; t0 += GSP_TH) {
    const int t = t0 + tid;
    const bool in = t < T;
    const int id = in ? ids[t] : -1;
    const int before_id = (in && t > 0) ? ids[t - 1] : -1;
    const bool keep = in && id != before_id && id != blank;
    const unsigned long long m = __ballot(keep);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wave_total[wave] = __popcll(m);
    __syncthreads();
    int off = carry_s;
    for (int w = 0; w < wave; ++w) off += wave_total[w];
    if (keep) {
      float sum = lps[t];
      int end = t + 1;
      bool open = true;
      for (int n0 = t + 1; open && n0 < T; n0 += 8) {
        int idn[8];
        float lpn[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int q = min(n0 + u, T - 1); idn[u] = ids[q]; lpn[u] = lps[q]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          if (open && n0 + u < T && idn[u] == id) { sum += lpn[u]; end = n0 + u + 1; }
          else open = false;
        }
      }
      const int r = off + before;                  // r <= t: inside the row
      tok_o[r] = id;
      span_o[2 * r] = t;
      span_o[2 * r + 1] = end;
      logp_o[r] = sum;
    }
    __syncthreads();
    if (tid == GSP_TH - 1) carry_s = off + before + (keep ? 1 : 0);
    __syncthreads();
  }
  const int n = carry_s;
  for (int i = n + tid; i < n_frames; i += GSP_TH) { tok_o[i] = 0; span_o[2 * i] = 0; span_o[2 * i + 1] = 0; logp_o[i] = 0.f; }
  if (tid == 0) counts[b] = n;
}

}  // namespace ts

// ts_ctc_loss's thresholds (csrc/ctc.hip: ctc_states_per_thread / ctc_threads)
static int align_states_per_thread(int lmax) { return lmax <= 1024 ? 1 : (lmax <= 2048 ? 2 : 4); }
static int align_threads(int lmax) { const int spt = align_states_per_thread(lmax); return ((lmax + spt - 1) / spt + 63) / 64 * 64; }

// What ts_ctc_align launches, as a function of the tensor's time dimension and the label capacity alone; ts_ctc_align launches from this and
// ts_ctc_align_launch_config reports it.
struct AlignLaunch {
  int spt, threads, nwt;
  bool bp_lds;
  size_t lds;
};
static int align_launch_config(int n_frames, int s_max, AlignLaunch* c) {
  if (n_frames <= 0 || s_max < 0) return TS_EINVAL;
  if (s_max > 2047) return TS_EUNSUPPORTED;
  const int lmax = 2 * s_max + 1;
  c->spt = align_states_per_thread(lmax);
  c->threads = align_threads(lmax);
  c->nwt = c->spt * c->threads / 64;
  const size_t rows = ((size_t)2 * (lmax + 4) + lmax) * sizeof(float) + ts::ALIGN_RED_BYTES;     // at most 49 KiB
  const size_t bp = (size_t)n_frames * c->nwt * sizeof(ulonglong2);
  c->bp_lds = rows + bp <= ts::ALIGN_LDS_MAX;
  c->lds = c->bp_lds ? rows + bp : rows;
  return TS_OK;
}

extern "C" int ts_ctc_align_abi_version(void) { return TS_CTC_ALIGN_ABI_VERSION; }

extern "C" int ts_ctc_align_launch_config(int32_t n_frames, int32_t s_max, int32_t* states_per_thread, int32_t* threads, int32_t* bp_in_lds,
                                          int32_t* lds_bytes) {
  if (!states_per_thread || !threads || !bp_in_lds || !lds_bytes) return TS_EINVAL;
  AlignLaunch c{};
  const int st = align_launch_config(n_frames, s_max, &c);
  if (st != TS_OK) return st;
  *states_per_thread = c.spt; *threads = c.threads; *bp_in_lds = c.bp_lds ? 1 : 0; *lds_bytes = (int32_t)c.lds;
  return TS_OK;
}

extern "C" int64_t ts_ctc_align_workspace_bytes(int32_t batch, int32_t n_frames, int32_t s_max) {
  if (batch <= 0) return TS_EINVAL;
  AlignLaunch c{};
  const int st = align_launch_config(n_frames, s_max, &c);
  if (st != TS_OK) return st;
  const int64_t bp = c.bp_lds ? 0 : (int64_t)batch * n_frames * c.nwt * (int64_t)sizeof(ulonglong2);
  return bp + (int64_t)batch * n_frames * (int64_t)(sizeof(int) + sizeof(float));
}

extern "C" int ts_ctc_align(const float* logits, int32_t batch, int32_t n_classes, int32_t n_frames, int32_t pitch, const int32_t* targets,
                            int32_t s_max, const int32_t* input_len, const int32_t* target_len, int32_t blank, int32_t* path, int32_t* spans,
                            float* span_logp, float* score, void* workspace, void* stream_) {
  using namespace ts;
  if (!logits || !targets || !input_len || !target_len || !path || !spans || !span_logp || !score || !workspace) return TS_EINVAL;
  if (batch <= 0 || n_classes <= 0 || n_frames <= 0 || pitch < n_frames || s_max < 0) return TS_EINVAL;
  if (blank < 0 || blank >= n_classes) return TS_EINVAL;
  AlignLaunch cfg{};
  const int cst = align_launch_config(n_frames, s_max, &cfg);
  if (cst != TS_OK) return cst;
  if (misaligned(workspace)) return TS_EUNSUPPORTED;
  TS_STREAM;
  AlignArgs a{};
  a.logits = logits; a.targets = targets; a.input_len = input_len; a.target_len = target_len;
  a.path = path; a.spans = spans; a.span_logp = span_logp; a.score = score;
  a.n_classes = n_classes; a.n_frames = n_frames; a.pitch = pitch; a.s_max = s_max; a.lmax = 2 * s_max + 1; a.blank = blank; a.nwt = cfg.nwt;
  char* ws = static_cast<char*>(workspace);
  a.bp = reinterpret_cast<ulonglong2*>(ws);
  if (!cfg.bp_lds) ws += (size_t)batch * n_frames * cfg.nwt * sizeof(ulonglong2);
  a.state = reinterpret_cast<int*>(ws);
  a.lp = reinterpret_cast<float*>(ws + (size_t)batch * n_frames * sizeof(int));
  const void* const fns[2][3] = {{reinterpret_cast<const void*>(ctc_align_kernel<1, false>), reinterpret_cast<const void*>(ctc_align_kernel<2, false>),
                                  reinterpret_cast<const void*>(ctc_align_kernel<4, false>)},
                                 {reinterpret_cast<const void*>(ctc_align_kernel<1, true>), reinterpret_cast<const void*>(ctc_align_kernel<2, true>),
                                  reinterpret_cast<const void*>(ctc_align_kernel<4, true>)}};
  const int which = cfg.spt == 1 ? 0 : (cfg.spt == 2 ? 1 : 2);
  const void* const fn = fns[cfg.bp_lds ? 1 : 0][which];
  static bool big_all[64][3] = {};                 // more than the default 64 KiB allowed: per (device, instantiation with the back-pointers in LDS)
  if (cfg.lds > 64 * 1024) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return TS_EINVAL;
    if (!big_all[dev][which]) {
      if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ALIGN_LDS_MAX) != hipSuccess) return TS_EUNSUPPORTED;
      big_all[dev][which] = true;
    }
  }
  void* params[] = {&a};
  const hipError_t e = hipLaunchKernel(fn, dim3(batch), dim3((unsigned)cfg.threads), params, cfg.lds, stream);
  if (e != hipSuccess) return (int)e;
  return hip_status(hipGetLastError());
}

extern "C" int64_t ts_ctc_greedy_spans_workspace_bytes(int32_t batch, int32_t n_frames) {
  if (batch <= 0 || n_frames <= 0) return TS_EINVAL;
  return (int64_t)batch * n_frames * (int64_t)(sizeof(int) + sizeof(float));
}

extern "C" int ts_ctc_greedy_spans(const float* logits, int32_t batch, int32_t n_classes, int32_t n_frames, int32_t pitch, const int32_t* input_len,
                                   int32_t blank, int32_t* tokens, int32_t* spans, float* span_logp, int32_t* counts, void* workspace,
                                   void* stream_) {
  if (!logits || !tokens || !spans || !span_logp || !counts || !workspace) return TS_EINVAL;
  if (batch <= 0 || n_classes <= 0 || n_frames <= 0 || pitch < n_frames) return TS_EINVAL;
  if (blank < 0 || blank >= n_classes) return TS_EINVAL;
  if (ts::misaligned(workspace, 3)) return TS_EUNSUPPORTED;
  TS_STREAM;
  int* const ids = static_cast<int*>(workspace);
  float* const lp = reinterpret_cast<float*>(ids + (size_t)batch * n_frames);
  hipLaunchKernelGGL(ts::ctc_greedy_spans_kernel, dim3(batch), dim3(ts::GSP_TH), 0, stream, logits, n_classes, n_frames, pitch, input_len, blank,
                     tokens, spans, span_logp, counts, ids, lp);
  return ts::hip_status(hipGetLastError());
}
