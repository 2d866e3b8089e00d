// CTC prefix beam search with n-best output, for gfx950.  No reference counterpart: the reference decodes greedily (module.py:98-101).
// ABI and the specification of the algorithm: include/thunder_speech_amd/ctc_beam.h.
//
// Three launches.
//   1. ctc_beam_cand_kernel, a wave per frame: the f64 normaliser and the token_cap largest non-blank logits.  The classes are spread over the
//      lanes; the k-th winner is the wave-wide maximum of the classes that come AFTER the (k-1)-th in the order (logit descending, class
//      ascending), so nothing is marked and V is never scanned serially: token_cap rounds of V / 64 loads per lane and 6 shuffle steps.
//   2. ctc_beam_search_kernel, a workgroup per utterance, a thread per RANKED candidate, two LDS-only barriers per frame:
//        a. child threads form their mass and look for their prefix in the beam (hash compare against the W beam hashes, two per 16-byte
//           broadcast LDS read): a child that is in the beam already is no candidate.  Its mass is formed by the STAY thread of that slot, which
//           finds its last token among the frame's records and its parent prefix in the beam (every entry carries its parent's hash) -- so the
//           merge needs no atomics, no extra barrier, and it also happens for the children that get no thread (below).  p[last] comes from the
//           frame's per-class row (up to BEAM_ROW classes); beyond, only a last token outside the frame's candidates costs the stay thread a
//           logit load and an f64 exp -- off the mass chain either way.  Every thread publishes its key;
//        b. COUNTING RANK: every thread counts the keys that beat its own -- on the keys' high words, four per 16-byte broadcast LDS read, and
//           exactly (key bits, then candidate order) only where a high word is shared by two candidates that may be kept.  A thread with rank < W writes
//           its entry to slot `rank` of the other beam buffer and, if it is a child, trie node 1 + t W + rank.  Zero keys rank last among
//           themselves, so every slot is written in every frame and nothing is cleared.
//      Why counting rank and not a bitonic sort or a radix select: the candidate set is small once it is pruned (below), the rank IS the slot,
//      ties cost one extra compare in candidate order, and it takes one barrier where a bitonic network over 512 keys takes 45 and a radix
//      select over the 63 key bits takes one per digit plus a histogram (with LDS atomics, which this file does without).
//      The pruning that makes it small, exact: the beam is stored in rank order, so tot_i' >= tot_i for slots i' < i, and the frame's classes are
//      stored by descending probability.  The child of slot i and the r-th class (r = 0 the most probable) is beaten by the children (i', r') with
//      i' < i, r' <= r that are not their slot's `c == last` child -- at least i (r + 1) - i = i r of them; one that merged is replaced by the stay
//      candidate it merged into, whose key is no smaller and which no other child maps to.  With i r >= W the child cannot be kept, so it gets no
//      thread: W (1 + H_W) candidates instead of W (token_cap + 1).
//      The frame records (and class rows) travel global -> register -> a four-slot LDS ring, requested three frames ahead of use.
//      The per-frame rescaling costs no barrier: the rank-0 thread leaves ilogb(key) next to the beam and every reader applies ldexp.
//   3. ctc_beam_backtrace_kernel, a wave per hypothesis: lane 0 walks the parents (each node records its depth, so tokens land in forward
//      order), the other lanes zero the tail.
#include "ts_common.hpp"

#include "thunder_speech_amd/ctc_beam.h"

// the f64 products and sums below are the specification's, one rounding each: no contraction into fma, no reassociation.  (The quotient of
// beam_prob keeps the build's reciprocal-and-refine form; both kernels form every probability through that one function.)
#pragma clang fp contract(off) reassociate(off)

#include "ctc_beam_cand.hpp"      // the limits, the hash, the LDS barrier and ctc_beam_cand_kernel, shared with csrc/ctc_beam_lm.hip

namespace ts {

// ranked children of beam slot i (k non-blank candidates per frame)
__host__ __device__ constexpr int beam_children(int i, int w, int k) { return i == 0 ? k : (k < (w + i - 1) / i ? k : (w + i - 1) / i); }

struct BeamArgs {
  const float* logits;      // [B][V][pitch]
  const int* input_len;
  const double* cp;         // workspace [B][n_frames][cap + 2]
  const int* cid;           // workspace [B][n_frames][cap + 2]
  const double* prow;       // workspace [B][n_frames][BEAM_ROW], written for n_classes <= BEAM_ROW
  int4* nodes;              // workspace [B][n_frames W + 1]: (parent node, token, frame, depth); node 0 is the root and is never stored
  int* fin;                 // workspace [B][BEAM_FIN]: trie node of final rank n
  int* lengths;             // [B][n_best]
  float* scores;            // [B][n_best]
  int* counts;              // [B]
  int n_classes, n_frames, pitch, W, cap, n_best, S;
};

__global__ __launch_bounds__(512) void ctc_beam_search_kernel(const BeamArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef unsigned long long u64;
  const int W = a.W, Wp = round_up(W, 8), K = a.cap + 1, R = K + 1, Re = beam_even(R), S = a.S, Se = round_up(S, 8);
  // two beam buffers (slot = rank): read from `cur`, written to the other
  double* const pb = reinterpret_cast<double*>(smem);            // [2][Wp]
  double* const pnb = pb + 2 * Wp;                               // [2][Wp]
  u64* const hs = reinterpret_cast<u64*>(pnb + 2 * Wp);          // [2][Wp]  ~0 for an empty slot
  u64* const phs = hs + 2 * Wp;                                  // [2][Wp]  hash of the prefix without its last token
  double* const skey = reinterpret_cast<double*>(phs + 2 * Wp);  // [Se]     the frame's keys, by thread
  double* const cpl = skey + Se;                                 // [4][Re]  the records of frame t in slot t & 3
  int* const last = reinterpret_cast<int*>(cpl + 4 * Re);        // [2][Wp]  -1 for the empty prefix
  int* const len = last + 2 * Wp;                                // [2][Wp]  -1 for an empty slot
  int* const node = len + 2 * Wp;                                // [2][Wp]
  unsigned* const sord = reinterpret_cast<unsigned*>(node + 2 * Wp);   // [Se]  candidate order of the frame's keys
  unsigned* const skhi = sord + Se;                              // [Se]     high words of the frame's keys
  int* const cidl = reinterpret_cast<int*>(skhi + Se);           // [4][Re]
  int* const esh = cidl + 4 * Re;                                // [2]      ilogb of the largest key of the buffer: readers scale by 2^-esh
  double* const prl = reinterpret_cast<double*>(esh + 4);        // [4][BEAM_ROW]  the frame's probabilities by class (n_classes <= BEAM_ROW)
  const int b = blockIdx.x, tid = threadIdx.x;
  int T = a.input_len ? a.input_len[b] : a.n_frames;
  T = T < 0 ? 0 : (T > a.n_frames ? a.n_frames : T);
  const float* const lg = a.logits + (size_t)b * a.n_classes * a.pitch;
  int4* const nodes = a.nodes + (size_t)b * ((size_t)a.n_frames * W + 1);

  // the thread's candidate: tid < W the stay candidate of slot tid; W <= tid < S the child of slot pi and the pr-th most probable class
  int pi = -1, pr = 0;
  if (tid >= W && tid < S) {
    int s = tid - W;
    for (int i = 0; i < W; ++i) {
      const int n = beam_children(i, W, K - 1);
      if (s < n) { pi = i; pr = s; break; }
      s -= n;
    }
  }
  // every thread prefetches a record (the threads beyond the R records of a frame read the last one again): all loads unconditional, so the
  // compiler counts them and a chunk holds no full vector-memory wait on their account (csrc/ctc_align.hip)
  const size_t rec0 = (size_t)b * a.n_frames * R + min(tid, R - 1);
  const bool full = a.n_classes <= BEAM_ROW;          // else the row loads below read the records again and nothing uses them
  const double* const rowp = full ? a.prow + (size_t)b * a.n_frames * BEAM_ROW + min(tid, BEAM_ROW - 1) : a.cp + rec0;
  const int rstride = full ? BEAM_ROW : R;
  for (int j = tid; j < 2 * Wp; j += blockDim.x) {
    const bool root = j == 0;
    pb[j] = root ? 1.0 : 0.0; pnb[j] = 0.0; hs[j] = root ? 0ull : ~0ull; phs[j] = ~0ull; last[j] = -1; len[j] = root ? 0 : -1; node[j] = 0;
  }
  for (int j = S + tid; j < Se; j += blockDim.x) { skey[j] = 0.0; skhi[j] = 0u; sord[j] = 0xffffffffu; }   // the pad key beats nothing: 0 with the last order
  if (tid < 2) esh[tid] = 0;
  // The records travel global -> register -> LDS ring, one step per frame: frame t writes the record of frame t + 2 (requested a frame
  // earlier) into slot (t + 2) & 3 and requests that of frame t + 3.  One copy of the step in the code, nothing to wait for inside it.
  int pend_id = 0;
  double pend_p = 0.0, pend_row = 0.0;
  auto request = [&](int f) {                          // clamped: loads of frames the pre-pass wrote
    const size_t fr = (size_t)min(f, T - 1);
    pend_id = a.cid[rec0 + fr * R];
    pend_p = a.cp[rec0 + fr * R];
    pend_row = rowp[fr * rstride];
  };
  auto deliver = [&](int f) {
    const int slot = f & 3;
    if (tid < R) { cidl[slot * Re + tid] = pend_id; cpl[slot * Re + tid] = pend_p; }
    if (tid < BEAM_ROW) prl[slot * BEAM_ROW + tid] = pend_row;
  };
  if (T > 0) {
    request(0); deliver(0);
    request(1); deliver(1);
    request(2);
  }
  __syncthreads();

  int esum = 0;
  const u64* const skeyb = reinterpret_cast<const u64*>(skey);
  // one frame
  auto step = [&](const int t) {
    const int cur = t & 1, nxt = cur ^ 1;
    const double* const cpb = pb + cur * Wp; const double* const cpnb = pnb + cur * Wp; const u64* const chs = hs + cur * Wp;
    const u64* const cphs = phs + cur * Wp;
    const int* const clast = last + cur * Wp; const int* const clen = len + cur * Wp; const int* const cnode = node + cur * Wp;
    const int* const ids = cidl + (t & 3) * Re; const double* const ps = cpl + (t & 3) * Re;
    const int e = esh[cur];
    esum += e;
    // ---- a. masses, merge detection, keys ----
    double npb = 0.0, npnb = 0.0, key = 0.0;
    unsigned ord = (unsigned)tid;
    int c = -2, xlen = -1, xlast = -1;
    u64 xhash = ~0ull, xph = ~0ull, want = ~0ull;
    if (tid < W) {
      xlast = clast[tid]; xlen = clen[tid]; xhash = chs[tid]; xph = cphs[tid];
      want = xph;                                      // the parent prefix, if it is in the beam
    } else if (pi >= 0) {
      c = ids[1 + pr];
      xph = chs[pi]; xhash = beam_mix(xph, c); xlen = clen[pi] + 1; xlast = c;
      want = xhash;                                    // the child's own prefix, if it is in the beam
    }
    // the beam slot whose hash is `want`: all reads first, no branch (an empty slot's hash is ~0; the lengths are compared below)
    int hit = -1;
    for (int j = 0; j < Wp; j += 8) {
      const ulonglong2 h0 = *reinterpret_cast<const ulonglong2*>(chs + j), h1 = *reinterpret_cast<const ulonglong2*>(chs + j + 2);
      const ulonglong2 h2 = *reinterpret_cast<const ulonglong2*>(chs + j + 4), h3 = *reinterpret_cast<const ulonglong2*>(chs + j + 6);
      hit = h0.x == want ? j : hit; hit = h0.y == want ? j + 1 : hit; hit = h1.x == want ? j + 2 : hit; hit = h1.y == want ? j + 3 : hit;
      hit = h2.x == want ? j + 4 : hit; hit = h2.y == want ? j + 5 : hit; hit = h3.x == want ? j + 6 : hit; hit = h3.y == want ? j + 7 : hit;
    }
    if (tid < W) {
      const double xb = ldexp(cpb[tid], -e), xnb = ldexp(cpnb[tid], -e);
      int ri = 0;                                      // the record of the last token, if it is a candidate of the frame
#pragma unroll 4
      for (int r = 1; r < K; ++r) ri = ids[r] == xlast ? r : ri;
      const bool found = ri > 0 && xlen >= 1;
      double pl = found ? ps[ri] : 0.0, merged = 0.0;
      if (found && hit >= 0 && clen[hit] == xlen - 1) {
        // (parent prefix, last token) is a child of this frame: its mass belongs to this stay candidate
        const double ib = ldexp(cpb[hit], -e), inb = ldexp(cpnb[hit], -e);
        merged = (xlast == clast[hit] ? ib : ib + inb) * pl;
      }
      if (full) pl = xlen >= 1 ? prl[(t & 3) * BEAM_ROW + min(max(xlast, 0), BEAM_ROW - 1)] : 0.0;
      else if (!found && xlen >= 1 && xnb > 0.0)
        pl = beam_prob(lg[(size_t)min(max(xlast, 0), a.n_classes - 1) * a.pitch + t], __int_as_float(ids[K]), ps[K]);
      npb = (xb + xnb) * ps[0];
      npnb = xnb * pl + merged;
      key = npb + npnb;
    } else if (pi >= 0) {
      const double xb = ldexp(cpb[pi], -e), xnb = ldexp(cpnb[pi], -e);
      const double mass = (c == clast[pi] ? xb : xb + xnb) * ps[1 + pr];
      // in the beam already: the stay candidate of that slot has taken the mass
      const bool in_beam = hit >= 0 && clen[hit] == xlen && clast[hit] == c;
      npnb = in_beam ? 0.0 : mass;
      key = npnb;
      ord = 0x80000000u | ((unsigned)pi << 25) | (c >= 0 ? (unsigned)c : (1u << 24) + (unsigned)pr);   // (parent slot, class); unique without a class too
    }
    if (tid < S) { skey[tid] = key; skhi[tid] = (unsigned)((u64)__double_as_longlong(key) >> 32); sord[tid] = ord; }
    beam_lds_barrier();
    // ---- b. counting rank; the kept candidates become the next beam ----
    // keys are non-negative, so their bit patterns order them: x beats y if key_x > key_y, or the keys are equal and x comes first.  The high
    // words decide almost always (two keys share one only within 2^-20 of each other, or as zeros): count on them first, 8 per two LDS reads,
    // and run the exact count only for a thread whose high word is shared and which may still be kept
    const u64 kb = (u64)__double_as_longlong(key);
    const unsigned khi = (unsigned)(kb >> 32);
    int rank = 0, same = 0;
    for (int s = 0; s < Se; s += 8) {
      const uint4 h0 = *reinterpret_cast<const uint4*>(skhi + s), h1 = *reinterpret_cast<const uint4*>(skhi + s + 4);
      rank += (int)(h0.x > khi) + (int)(h0.y > khi) + (int)(h0.z > khi) + (int)(h0.w > khi) + (int)(h1.x > khi) + (int)(h1.y > khi) +
              (int)(h1.z > khi) + (int)(h1.w > khi);
      same += (int)(h0.x == khi) + (int)(h0.y == khi) + (int)(h0.z == khi) + (int)(h0.w == khi) + (int)(h1.x == khi) + (int)(h1.y == khi) +
              (int)(h1.z == khi) + (int)(h1.w == khi);
    }
    if (tid < S && rank < W && same > 1) {             // `same` counts the thread's own key
      rank = 0;
      for (int s = 0; s < Se; s += 8) {
        const ulonglong2 k0 = *reinterpret_cast<const ulonglong2*>(skeyb + s), k1 = *reinterpret_cast<const ulonglong2*>(skeyb + s + 2);
        const ulonglong2 k2 = *reinterpret_cast<const ulonglong2*>(skeyb + s + 4), k3 = *reinterpret_cast<const ulonglong2*>(skeyb + s + 6);
        const uint4 o0 = *reinterpret_cast<const uint4*>(sord + s), o1 = *reinterpret_cast<const uint4*>(sord + s + 4);
        rank += (int)((k0.x > kb) | ((k0.x == kb) & (o0.x < ord))) + (int)((k0.y > kb) | ((k0.y == kb) & (o0.y < ord)));
        rank += (int)((k1.x > kb) | ((k1.x == kb) & (o0.z < ord))) + (int)((k1.y > kb) | ((k1.y == kb) & (o0.w < ord)));
        rank += (int)((k2.x > kb) | ((k2.x == kb) & (o1.x < ord))) + (int)((k2.y > kb) | ((k2.y == kb) & (o1.y < ord)));
        rank += (int)((k3.x > kb) | ((k3.x == kb) & (o1.z < ord))) + (int)((k3.y > kb) | ((k3.y == kb) & (o1.w < ord)));
      }
    }
    // the records first: their wait covers the loads and the node store of the frame before, all a frame old; behind this frame's node store
    // it would wait for that store's round trip in every frame
    deliver(t + 2);
    request(t + 3);
    if (tid < S && rank < W) {
      const bool live = key > 0.0;
      const int at = nxt * Wp + rank;
      int nid = tid < W ? cnode[tid] : 0;
      if (live && tid >= W) {
        nid = 1 + t * W + rank;
        nodes[nid] = make_int4(cnode[pi], c, t, xlen);
      }
      pb[at] = live ? npb : 0.0; pnb[at] = live ? npnb : 0.0; hs[at] = live ? xhash : ~0ull; phs[at] = live ? xph : ~0ull;
      last[at] = live ? xlast : -1; len[at] = live ? xlen : -1; node[at] = live ? nid : 0;
      if (rank == 0) esh[nxt] = live ? ilogb(key) : 0;
    }
    beam_lds_barrier();
  };
  for (int t = 0; t < T; ++t) step(t);
  // the final beam is in rank order; its masses still carry 2^esum (esh of the final buffer is not applied)
  const int fb = (T & 1) * Wp;
  if (tid < a.n_best) {
    const double tot = pb[fb + tid] + pnb[fb + tid];
    const bool live = tot > 0.0;
    a.scores[(size_t)b * a.n_best + tid] = live ? (float)(log(tot) + (double)esum * 0.693147180559945309417232121458) : BEAM_NEG_INF;
    a.lengths[(size_t)b * a.n_best + tid] = live ? len[fb + tid] : 0;
    a.fin[(size_t)b * BEAM_FIN + tid] = live ? node[fb + tid] : 0;
  }
  if (tid == 0) {
    int n = 0;
    for (int j = 0; j < a.n_best; ++j) n += (pb[fb + j] + pnb[fb + j] > 0.0) ? 1 : 0;
    a.counts[b] = n;
  }
}

__global__ __launch_bounds__(64) void ctc_beam_backtrace_kernel(const int4* __restrict__ nodes_all, const int* __restrict__ fin,
                                                                const int* __restrict__ lengths, int n_frames, int W, int n_best,
                                                                int* __restrict__ tokens, int* __restrict__ frames) {
  const int n = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const int4* const nodes = nodes_all + (size_t)b * ((size_t)n_frames * W + 1);
  int* const tok = tokens + ((size_t)b * n_best + n) * n_frames;
  int* const frm = frames + ((size_t)b * n_best + n) * n_frames;
  const int L = min(max(lengths[(size_t)b * n_best + n], 0), n_frames);
  for (int p = L + lane; p < n_frames; p += 64) { tok[p] = 0; frm[p] = 0; }
  if (lane == 0) {
    int id = fin[(size_t)b * BEAM_FIN + n];
    const int last_id = n_frames * W;
    for (int p = L - 1; p >= 0; --p) {
      int4 nd = make_int4(0, 0, 0, 0);
      if (id >= 1 && id <= last_id) nd = nodes[id];
      tok[p] = nd.y;
      frm[p] = nd.z;
      id = nd.x;
    }
  }
}

}  // namespace ts

// What ts_ctc_beam_search launches, as a function of the class count and the two widths alone; the launcher launches from this and
// ts_ctc_beam_launch_config reports it.
struct BeamLaunch {
  int cap, cands, threads;
  size_t lds;
};
static int beam_launch_config(int n_classes, int beam_width, int token_cap, BeamLaunch* c) {
  if (n_classes <= 0 || beam_width < 1 || token_cap < 1) return TS_EINVAL;
  if (beam_width > ts::BEAM_MAX || token_cap > ts::BEAM_MAX || n_classes > (1 << 24)) return TS_EUNSUPPORTED;
  c->cap = token_cap < n_classes - 1 ? token_cap : n_classes - 1;
  c->cands = beam_width;
  for (int i = 0; i < beam_width; ++i) c->cands += ts::beam_children(i, beam_width, c->cap);
  c->threads = ts::round_up(c->cands, 64);             // at most 64 + 64 + sum ceil(64 / i) = 471 candidates: 512 threads
  c->lds = (size_t)88 * ts::round_up(beam_width, 8) + (size_t)16 * ts::round_up(c->cands, 8) + (size_t)48 * ts::beam_even(c->cap + 2) + 16 + 32 * ts::BEAM_ROW;
  return TS_OK;
}

extern "C" int ts_ctc_beam_abi_version(void) { return TS_CTC_BEAM_ABI_VERSION; }

extern "C" int ts_ctc_beam_launch_config(int32_t n_classes, int32_t beam_width, int32_t token_cap, int32_t* threads, int32_t* lds_bytes,
                                         int32_t* candidates) {
  if (!threads || !lds_bytes || !candidates) return TS_EINVAL;
  BeamLaunch c{};
  const int st = beam_launch_config(n_classes, beam_width, token_cap, &c);
  if (st != TS_OK) return st;
  *threads = c.threads; *lds_bytes = (int32_t)c.lds; *candidates = c.cands;
  return TS_OK;
}

extern "C" int64_t ts_ctc_beam_workspace_bytes(int32_t batch, int32_t n_frames, int32_t beam_width, int32_t token_cap) {
  if (batch <= 0 || n_frames <= 0 || beam_width < 1 || token_cap < 1) return TS_EINVAL;
  if (beam_width > ts::BEAM_MAX || token_cap > ts::BEAM_MAX) return TS_EUNSUPPORTED;
  return (int64_t)batch * (16 * ((int64_t)n_frames * beam_width + 1) + 12 * (int64_t)n_frames * (token_cap + 2) + 8 * ts::BEAM_ROW * (int64_t)n_frames + 4 * ts::BEAM_FIN);
}

extern "C" int ts_ctc_beam_search(const float* logits, int32_t batch, int32_t n_classes, int32_t n_frames, int32_t pitch, const int32_t* input_len,
                                  int32_t blank, int32_t beam_width, int32_t token_cap, int32_t n_best, int32_t* tokens, int32_t* frames,
                                  int32_t* lengths, float* scores, int32_t* counts, void* workspace, void* stream_) {
  using namespace ts;
  if (!logits || !tokens || !frames || !lengths || !scores || !counts || !workspace) return TS_EINVAL;
  if (batch <= 0 || n_classes <= 0 || n_frames <= 0 || pitch < n_frames) return TS_EINVAL;
  if (blank < 0 || blank >= n_classes) return TS_EINVAL;
  if (n_best < 1) return TS_EINVAL;
  BeamLaunch cfg{};
  const int cst = beam_launch_config(n_classes, beam_width, token_cap, &cfg);
  if (cst != TS_OK) return cst;
  if (n_best > BEAM_MAX) return TS_EUNSUPPORTED;
  if (n_best > beam_width) return TS_EINVAL;
  if (misaligned(workspace)) return TS_EUNSUPPORTED;
  if ((int64_t)n_frames * beam_width + 1 > 0x7fffffff) return TS_EUNSUPPORTED;     // trie node ids are int32
  TS_STREAM;
  // workspace: nodes (16 bytes each), the records' probabilities (8), the class rows (8), the records' ids (4), the final nodes (4); laid out for the clamped token_cap,
  // inside the ts_ctc_beam_workspace_bytes of the caller's
  char* ws = static_cast<char*>(workspace);
  BeamArgs a{};
  a.nodes = reinterpret_cast<int4*>(ws);
  ws += (size_t)batch * ((size_t)n_frames * beam_width + 1) * sizeof(int4);
  double* const cp = reinterpret_cast<double*>(ws);
  ws += (size_t)batch * n_frames * (cfg.cap + 2) * sizeof(double);
  double* const prow = reinterpret_cast<double*>(ws);
  ws += (size_t)batch * n_frames * BEAM_ROW * sizeof(double);
  int* const cid = reinterpret_cast<int*>(ws);
  ws += (size_t)batch * n_frames * (cfg.cap + 2) * sizeof(int);
  a.fin = reinterpret_cast<int*>(ws);
  a.logits = logits; a.input_len = input_len; a.cp = cp; a.cid = cid; a.prow = prow; a.lengths = lengths; a.scores = scores; a.counts = counts;
  a.n_classes = n_classes; a.n_frames = n_frames; a.pitch = pitch; a.W = beam_width; a.cap = cfg.cap; a.n_best = n_best; a.S = cfg.cands;
  hipLaunchKernelGGL(ctc_beam_cand_kernel, dim3((unsigned)((n_frames + 3) / 4), (unsigned)batch), dim3(256), 0, stream, logits, n_classes, n_frames,
                     pitch, input_len, blank, cfg.cap, cp, cid, prow);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(ctc_beam_search_kernel, dim3((unsigned)batch), dim3((unsigned)cfg.threads), cfg.lds, stream, a);
  e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(ctc_beam_backtrace_kernel, dim3((unsigned)n_best, (unsigned)batch), dim3(64), 0, stream, a.nodes, a.fin, lengths, n_frames,
                     beam_width, n_best, tokens, frames);
  return hip_status(hipGetLastError());
}
