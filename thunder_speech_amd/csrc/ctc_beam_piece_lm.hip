// CTC prefix beam search over a sentencepiece vocabulary with a WORD-level n-gram LM, a lexicon trie over letters and hot words, for gfx950.  No
// reference counterpart.  ABI and the child rule: include_open/thunder_speech_amd/ctc_beam_piece_lm.h; the algorithm around it is that of
// include_open/thunder_speech_amd/ctc_beam_word_lm.h, and csrc/ctc_beam_word_lm.hip is the search whose structure this one keeps (left as it is:
// its kernel stays the one its tests and its profile know).
//
// Three launches.
//   1. ctc_beam_cand_kernel (csrc/ctc_beam_cand.hpp), the pre-pass of csrc/ctc_beam.hip, unchanged.
//   2. ctc_beam_piece_lm_search_kernel, a workgroup per utterance, a thread per candidate -- every child of every slot.  A beam entry carries the
//      word automaton's state and the lexicon state (trie node, 0 = root, -1 = outside the lexicon).  The LDS layout and the three LDS-only
//      barriers per frame are ctc_beam_word_lm.hip's:
//        a. a child thread forms its acoustic mass and then does the piece's work in two steps that every lane of a wave passes in the same
//           order, so that lanes diverge inside a step and meet again after it: FIRST the end of the pending word, for the word-start pieces
//           that have one (the word's lookup in the word automaton -- binary search of a state's arcs, a back-off arc where the word is missing,
//           one f64 product per arc met -- then the hot-word factor or the OOV factor); THEN the piece's letters through the trie, one binary
//           search of a node's edges per letter (global memory, read-only, L2-resident: the tables of a served LM are a few MiB and every
//           workgroup reads the same ones), until the piece ends or the spelling leaves the trie, where it pays oov_factor once.  A wave waits
//           for its longest piece (sentencepiece pieces are 1 to about 8 letters) and, in the first step, for its deepest back-off walk (the
//           LM's order at most); lanes whose candidate is dead (mass 0) skip both.  Then the child looks for its prefix in the beam (hash
//           compare); a child that is in the beam already leaves its mass in `merged` of that slot: one child at most writes a slot -- no
//           atomics;
//        b. the stay threads add the merged mass and every thread publishes its key;
//        c. counting rank.  A thread with rank < W writes slot `rank` of the other beam buffer and, if it is a child, trie node 1 + t W + rank.
//      With n_classes > BEAM_ROW (every sentencepiece model: Citrinet has 1025) the pre-pass leaves no row of probabilities, and a stay
//      candidate whose last token is not among the frame's records reads its logit and forms the probability from the frame's normaliser.
//      After the last frame each of the W entries takes its pending word and its </s> factor, and the W keys are ranked once more.
//   3. ctc_beam_piece_lm_backtrace_kernel, a wave per hypothesis: lane 0 walks the parents, leaving the node ids in the `frames` row, then walks
//      the row forward: the frame of each node and the f64 sum of the nodes' log10 LM scores in forward order.
#include "ts_common.hpp"

#include "thunder_speech_amd/ctc_beam_piece_lm.h"

// the f64 products and sums below are the specification's, one rounding each: no contraction into fma, no reassociation
#pragma clang fp contract(off) reassociate(off)

#include "ctc_beam_cand.hpp"

namespace ts {

constexpr int BEAM_PIECE_CANDS = 1024;                // candidates (= threads) at most

struct BeamPieceNode {                                // second half of a trie node
  double log10;                                       // unweighted log10 LM score of the node: the lookup of the word that the piece ended, else 0
  int state, lex;                                     // word-automaton state and lexicon state entered
};

struct BeamPieceArgs {
  const float* logits;      // [B][V][pitch]
  const int* input_len;
  const double* cp;         // workspace [B][n_frames][cap + 2]
  const int* cid;           // workspace [B][n_frames][cap + 2]
  const double* prow;       // workspace [B][n_frames][BEAM_ROW], written for n_classes <= BEAM_ROW
  int4* nodes;              // workspace [B][n_frames W + 1]: (parent node, token, frame, depth); node 0 is the root and is never stored
  BeamPieceNode* nodes_lm;  // workspace [B][n_frames W + 1]
  int* fin;                 // workspace [B][BEAM_FIN]: trie node of final rank n
  double* fin_end;          // workspace [B][BEAM_FIN]: log10 of the pending word + log10 P(</s>) applied to final rank n (0 without)
  int* lengths;             // [B][n_best]
  float* scores;            // [B][n_best]
  int* counts;              // [B]
  // the word automaton (thunder_speech_amd/ctc_beam_lm.h)
  const int* arc_begin; const int* arc_class; const int* arc_next; const double* arc_factor; const double* arc_log10;
  const int* bo_next; const double* bo_factor; const double* bo_log10; const double* eos_factor; const double* eos_log10;
  // the lexicon over letters (thunder_speech_amd/ctc_beam_word_lm.h)
  const int* edge_begin; const int* edge_class; const int* edge_next; const int* node_word; const int* word_class;
  const double* word_factor; const double* oov_factor;
  // the pieces (thunder_speech_amd/ctc_beam_piece_lm.h)
  const int* piece_begin; const int* piece_letter; const int* piece_kind;
  int n_states, n_arcs, start_state, eos;
  int n_nodes, n_edges, n_words, unk_class;
  int n_piece_letters;
  int n_classes, n_frames, pitch, W, cap, n_best, S;
};

// The lookup of ctc_beam_lm.h for class c of the word automaton: from state s down the back-off arcs to the first state that has an arc of class
// c; one product and one sum per arc met, in the order met.  A class that state 0 lacks drops the candidate (mass 0).
__device__ __forceinline__ void beam_piece_lookup(const BeamPieceArgs& a, int s, const int c, double& mass, double& lmlog, int& state) {
  const int last_state = a.n_states - 1;
  s = min(max(s, 0), last_state);
  bool done = !(mass > 0.0);
  while (!done) {
    int lo = min(max(a.arc_begin[s], 0), a.n_arcs), hi = min(max(a.arc_begin[s + 1], lo), a.n_arcs);
    const int end = hi;
    while (lo < hi) {                                  // the first arc of the state with class >= c
      const int mid = (lo + hi) >> 1;
      if (a.arc_class[mid] < c) lo = mid + 1; else hi = mid;
    }
    if (lo < end && a.arc_class[lo] == c) {
      mass = mass * a.arc_factor[lo];
      lmlog = lmlog + a.arc_log10[lo];
      state = min(max(a.arc_next[lo], 0), last_state);
      done = true;
    } else if (s == 0) {
      mass = 0.0;                                      // state 0 has no arc of the class: no LM entry at all
      done = true;
    } else {
      mass = mass * a.bo_factor[s];
      lmlog = lmlog + a.bo_log10[s];
      const int ns = min(max(a.bo_next[s], 0), last_state);
      s = ns < s ? ns : 0;                             // back-off arcs lead to lower states (ctc_lm.py numbers states by length): the walk ends
    }
  }
}

// The end of a word at lexicon state x != 0, from word state s: the word's class (unk_class without a word) is looked up, then the word's
// hot-word factor, or -- for a node that is not terminal -- the OOV factor (x = -1 paid it when the spelling left the trie).
__device__ __forceinline__ void beam_piece_word_end(const BeamPieceArgs& a, const int s, const int x, double& mass, double& lmlog, int& state) {
  int w = x > 0 ? a.node_word[min(x, a.n_nodes - 1)] : -1;
  w = w < a.n_words ? w : -1;
  const int cls = w >= 0 ? a.word_class[w] : a.unk_class;
  beam_piece_lookup(a, s, cls, mass, lmlog, state);
  if (w >= 0) mass = mass * a.word_factor[w];
  else if (x > 0) mass = mass * a.oov_factor[0];
}

// The letters j0 <= j < j1 of a piece from lexicon state x >= 0: an edge per letter, until the piece ends or node x has no edge of the letter;
// there the spelling leaves the lexicon (x = -1) and the word pays, once.
__device__ __forceinline__ void beam_piece_letters(const BeamPieceArgs& a, int j, const int j1, int& x, double& mass) {
  const int last_node = a.n_nodes - 1;
  for (; j < j1 && x >= 0; ++j) {
    const int letter = a.piece_letter[j];
    int lo = min(max(a.edge_begin[x], 0), a.n_edges), hi = min(max(a.edge_begin[x + 1], lo), a.n_edges);
    const int end = hi;
    while (lo < hi) {                                  // the first edge of the node with letter >= this one
      const int mid = (lo + hi) >> 1;
      if (a.edge_class[mid] < letter) lo = mid + 1; else hi = mid;
    }
    if (lo < end && a.edge_class[lo] == letter) {
      x = min(max(a.edge_next[lo], 0), last_node);
    } else {
      x = -1;
      mass = mass * a.oov_factor[0];
    }
  }
}

__global__ __launch_bounds__(1024) void ctc_beam_piece_lm_search_kernel(const BeamPieceArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef unsigned long long u64;
  const int W = a.W, Wp = round_up(W, 8), K = a.cap + 1, R = K + 1, Re = beam_even(R), S = a.S, Se = round_up(S, 8);
  // two beam buffers (slot = rank): read from `cur`, written to the other
  double* const pb = reinterpret_cast<double*>(smem);            // [2][Wp]
  double* const pnb = pb + 2 * Wp;                               // [2][Wp]
  u64* const hs = reinterpret_cast<u64*>(pnb + 2 * Wp);          // [2][Wp]  ~0 for an empty slot
  double* const merged = reinterpret_cast<double*>(hs + 2 * Wp); // [Wp]     mass of the child that merges into the slot; 0 between frames
  double* const skey = merged + Wp;                              // [Se]     the frame's keys, by thread
  double* const cpl = skey + Se;                                 // [4][Re]  the records of frame t in slot t & 3
  double* const prl = cpl + 4 * Re;                              // [4][BEAM_ROW]  the frame's probabilities by class (n_classes <= BEAM_ROW)
  int* const last = reinterpret_cast<int*>(prl + 4 * BEAM_ROW);  // [2][Wp]  -1 for the empty prefix
  int* const len = last + 2 * Wp;                                // [2][Wp]  -1 for an empty slot
  int* const node = len + 2 * Wp;                                // [2][Wp]
  int* const lms = node + 2 * Wp;                                // [2][Wp]  word-automaton state of the prefix
  int* const lxs = lms + 2 * Wp;                                 // [2][Wp]  lexicon state of the prefix: trie node, 0 the root, -1 outside
  unsigned* const sord = reinterpret_cast<unsigned*>(lxs + 2 * Wp);    // [Se]  candidate order of the frame's keys
  unsigned* const skhi = sord + Se;                              // [Se]     high words of the frame's keys
  int* const cidl = reinterpret_cast<int*>(skhi + Se);           // [4][Re]
  int* const esh = cidl + 4 * Re;                                // [2]      ilogb of the largest key of the buffer: readers scale by 2^-esh
  const int b = blockIdx.x, tid = threadIdx.x;
  int T = a.input_len ? a.input_len[b] : a.n_frames;
  T = T < 0 ? 0 : (T > a.n_frames ? a.n_frames : T);
  const float* const lg = a.logits + (size_t)b * a.n_classes * a.pitch;
  int4* const nodes = a.nodes + (size_t)b * ((size_t)a.n_frames * W + 1);
  BeamPieceNode* const nodes_lm = a.nodes_lm + (size_t)b * ((size_t)a.n_frames * W + 1);

  // the thread's candidate: tid < W the stay candidate of slot tid; W <= tid < S the child of slot pi and the pr-th most probable class
  const bool child = tid >= W && tid < S;
  const int pi = child ? (tid - W) / (K - 1) : -1, pr = child ? (tid - W) % (K - 1) : 0;
  // every thread prefetches a record (the threads beyond the R records of a frame read the last one again): all loads unconditional
  const size_t rec0 = (size_t)b * a.n_frames * R + min(tid, R - 1);
  const bool full = a.n_classes <= BEAM_ROW;          // else the row loads below read the records again and nothing uses them
  const double* const rowp = full ? a.prow + (size_t)b * a.n_frames * BEAM_ROW + min(tid, BEAM_ROW - 1) : a.cp + rec0;
  const int rstride = full ? BEAM_ROW : R;
  for (int j = tid; j < 2 * Wp; j += blockDim.x) {
    const bool root = j == 0;
    pb[j] = root ? 1.0 : 0.0; pnb[j] = 0.0; hs[j] = root ? 0ull : ~0ull; last[j] = -1; len[j] = root ? 0 : -1; node[j] = 0;
    lms[j] = root ? a.start_state : 0; lxs[j] = 0;
  }
  for (int j = tid; j < Wp; j += blockDim.x) merged[j] = 0.0;
  for (int j = S + tid; j < Se; j += blockDim.x) { skey[j] = 0.0; skhi[j] = 0u; sord[j] = 0xffffffffu; }   // the pad key beats nothing: 0 with the last order
  if (tid < 2) esh[tid] = 0;
  // The records travel global -> register -> LDS ring, one step per frame: frame t writes the record of frame t + 2 (requested a frame
  // earlier) into slot (t + 2) & 3 and requests that of frame t + 3.
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
  const int last_state = a.n_states - 1, last_node = a.n_nodes - 1, last_class = a.n_classes - 1;
  // one frame
  auto step = [&](const int t) {
    const int cur = t & 1, nxt = cur ^ 1;
    const double* const cpb = pb + cur * Wp; const double* const cpnb = pnb + cur * Wp; const u64* const chs = hs + cur * Wp;
    const int* const clast = last + cur * Wp; const int* const clen = len + cur * Wp; const int* const cnode = node + cur * Wp;
    const int* const clms = lms + cur * Wp; const int* const clxs = lxs + cur * Wp;
    const int* const ids = cidl + (t & 3) * Re; const double* const ps = cpl + (t & 3) * Re;
    const int e = esh[cur];
    esum += e;
    // ---- a. masses; a child ends the pending word if its piece starts one, walks its letters, and looks for its prefix in the beam ----
    double npb = 0.0, npnb = 0.0, key = 0.0, lmlog = 0.0;
    unsigned ord = (unsigned)tid;
    int c = -2, xlen = -1, xlast = -1, xstate = 0, xlex = 0;
    u64 xhash = ~0ull;
    if (tid < W) {
      xlast = clast[tid]; xlen = clen[tid]; xhash = chs[tid]; xstate = clms[tid]; xlex = clxs[tid];
      const double xb = ldexp(cpb[tid], -e), xnb = ldexp(cpnb[tid], -e);
      int ri = 0;                                      // the record of the last token, if it is a candidate of the frame
#pragma unroll 4
      for (int r = 1; r < K; ++r) ri = ids[r] == xlast ? r : ri;
      const bool found = ri > 0 && xlen >= 1;
      double pl = found ? ps[ri] : 0.0;
      if (full) pl = xlen >= 1 ? prl[(t & 3) * BEAM_ROW + min(max(xlast, 0), BEAM_ROW - 1)] : 0.0;
      else if (!found && xlen >= 1 && xnb > 0.0)       // many classes: the logit itself, with the frame's normaliser
        pl = beam_prob(lg[(size_t)min(max(xlast, 0), last_class) * a.pitch + t], __int_as_float(ids[K]), ps[K]);
      npb = (xb + xnb) * ps[0];
      npnb = xnb * pl;
    } else if (child) {
      c = ids[1 + pr];
      const double xb = ldexp(cpb[pi], -e), xnb = ldexp(cpnb[pi], -e);
      double mass = (c == clast[pi] ? xb : xb + xnb) * ps[1 + pr];
      xhash = beam_mix(chs[pi], c); xlen = clen[pi] + 1; xlast = c;
      ord = 0x80000000u | ((unsigned)pi << 25) | (c >= 0 ? (unsigned)c : (1u << 24) + (unsigned)pr);   // (parent slot, class); unique without a class too
      if (clen[pi] < 0 || c < 0) mass = 0.0;           // an empty slot, a record without a class
      xstate = min(max(clms[pi], 0), last_state);
      xlex = min(max(clxs[pi], -1), last_node);
      if (mass > 0.0) {
        const int cc = min(c, last_class);             // (c >= 0 here)
        const int kind = a.piece_kind[cc];
        const int j0 = min(max(a.piece_begin[cc], 0), a.n_piece_letters), j1 = min(max(a.piece_begin[cc + 1], j0), a.n_piece_letters);
        // step 1: a piece that starts a word ends the pending one (after none -- the start of a clip, a bare word-start piece before: nothing)
        if (kind == 1 && xlex != 0) {
          beam_piece_word_end(a, xstate, xlex, mass, lmlog, xstate);
          xlex = 0;
        }
        // step 2: the letters; a class without a spelling is one letter that no node has an edge for
        if (kind != 2) {
          beam_piece_letters(a, j0, j1, xlex, mass);
        } else if (xlex >= 0) {
          xlex = -1;
          mass = mass * a.oov_factor[0];
        }
      }
      // the beam slot that holds the child's prefix, if any (an empty slot's hash is ~0; length and last token are compared too)
      int hit = -1;
      for (int j = 0; j < Wp; j += 8) {
        const ulonglong2 h0 = *reinterpret_cast<const ulonglong2*>(chs + j), h1 = *reinterpret_cast<const ulonglong2*>(chs + j + 2);
        const ulonglong2 h2 = *reinterpret_cast<const ulonglong2*>(chs + j + 4), h3 = *reinterpret_cast<const ulonglong2*>(chs + j + 6);
        hit = h0.x == xhash ? j : hit; hit = h0.y == xhash ? j + 1 : hit; hit = h1.x == xhash ? j + 2 : hit; hit = h1.y == xhash ? j + 3 : hit;
        hit = h2.x == xhash ? j + 4 : hit; hit = h2.y == xhash ? j + 5 : hit; hit = h3.x == xhash ? j + 6 : hit; hit = h3.y == xhash ? j + 7 : hit;
      }
      const bool in_beam = hit >= 0 && clen[hit] == xlen && clast[hit] == c;
      if (in_beam) merged[hit] = mass;                 // one child at most per slot
      npnb = in_beam ? 0.0 : mass;
      key = npnb;
    }
    beam_lds_barrier();
    // ---- b. the stay candidates take the merged mass; keys ----
    if (tid < W) {
      npnb = npnb + merged[tid];
      merged[tid] = 0.0;
      key = npb + npnb;
    }
    if (tid < S) { skey[tid] = key; skhi[tid] = (unsigned)((u64)__double_as_longlong(key) >> 32); sord[tid] = ord; }
    beam_lds_barrier();
    // ---- c. counting rank; the kept candidates become the next beam ----
    // keys are non-negative, so their bit patterns order them: x beats y if key_x > key_y, or the keys are equal and x comes first
    const u64 kb = (u64)__double_as_longlong(key);
    const unsigned khi = (unsigned)(kb >> 32);
    int rank = 0, same = 0;
    auto count8 = [&](const int s) {
      const uint4 h0 = *reinterpret_cast<const uint4*>(skhi + s), h1 = *reinterpret_cast<const uint4*>(skhi + s + 4);
      rank += (int)(h0.x > khi) + (int)(h0.y > khi) + (int)(h0.z > khi) + (int)(h0.w > khi) + (int)(h1.x > khi) + (int)(h1.y > khi) +
              (int)(h1.z > khi) + (int)(h1.w > khi);
      same += (int)(h0.x == khi) + (int)(h0.y == khi) + (int)(h0.z == khi) + (int)(h0.w == khi) + (int)(h1.x == khi) + (int)(h1.y == khi) +
              (int)(h1.z == khi) + (int)(h1.w == khi);
    };
    if (Se <= 256) {
      for (int s = 0; s < Se; s += 8) count8(s);
    } else {
      // many candidates: in chunks of 64 keys, and a wave none of whose candidates can be kept any more stops counting (ctc_beam_lm.hip)
      for (int s0 = 0; s0 < Se; s0 += 64) {
        const int s1 = min(s0 + 64, Se);
#pragma unroll 8
        for (int s = s0; s < s1; s += 8) count8(s);
        if (__all(rank >= W)) break;                   // wave-uniform
      }
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
    deliver(t + 2);
    request(t + 3);
    if (tid < S && rank < W) {
      const bool live = key > 0.0;
      const int at = nxt * Wp + rank;
      int nid = tid < W ? cnode[tid] : 0;
      if (live && tid >= W) {
        nid = 1 + t * W + rank;
        nodes[nid] = make_int4(cnode[pi], c, t, xlen);
        BeamPieceNode nl; nl.log10 = lmlog; nl.state = xstate; nl.lex = xlex;
        nodes_lm[nid] = nl;
      }
      pb[at] = live ? npb : 0.0; pnb[at] = live ? npnb : 0.0; hs[at] = live ? xhash : ~0ull;
      last[at] = live ? xlast : -1; len[at] = live ? xlen : -1; node[at] = live ? nid : 0; lms[at] = live ? xstate : 0; lxs[at] = live ? xlex : 0;
      if (rank == 0) esh[nxt] = live ? ilogb(key) : 0;
    }
    beam_lds_barrier();
  };
  for (int t = 0; t < T; ++t) step(t);
  // the final beam is in rank order; its masses still carry 2^esum (esh of the final buffer is not applied).  Each entry takes its pending word
  // and, with </s>, that factor; then one more ranking of the W keys, each thread against all (equal keys by slot)
  const int fb = (T & 1) * Wp;
  double fkey = 0.0, fend = 0.0;
  if (tid < W) {
    fkey = pb[fb + tid] + pnb[fb + tid];
    if (fkey > 0.0) {
      int s = min(max(lms[fb + tid], 0), last_state);
      const int x = min(max(lxs[fb + tid], -1), last_node);
      if (x != 0) beam_piece_word_end(a, s, x, fkey, fend, s);
      if (a.eos && fkey > 0.0) {
        fkey = fkey * a.eos_factor[s];
        fend = fend + a.eos_log10[s];
      }
    }
    skey[tid] = fkey;
  }
  __syncthreads();
  if (tid < W) {
    int rank = 0;
    for (int j = 0; j < W; ++j) {
      const double kj = skey[j];
      rank += (int)((kj > fkey) | ((kj == fkey) & (j < tid)));
    }
    if (rank < a.n_best) {
      const bool live = fkey > 0.0;
      a.scores[(size_t)b * a.n_best + rank] = live ? (float)(log(fkey) + (double)esum * 0.693147180559945309417232121458) : BEAM_NEG_INF;
      a.lengths[(size_t)b * a.n_best + rank] = live ? len[fb + tid] : 0;
      a.fin[(size_t)b * BEAM_FIN + rank] = live ? node[fb + tid] : -1;          // -1: no hypothesis of this rank
      a.fin_end[(size_t)b * BEAM_FIN + rank] = live ? fend : 0.0;
    }
  }
  if (tid == 0) {
    int n = 0;
    for (int j = 0; j < W; ++j) n += skey[j] > 0.0 ? 1 : 0;
    a.counts[b] = n < a.n_best ? n : a.n_best;
  }
}

__global__ __launch_bounds__(64) void ctc_beam_piece_lm_backtrace_kernel(const int4* __restrict__ nodes_all, const BeamPieceNode* __restrict__ nodes_lm_all,
                                                                         const int* __restrict__ fin, const double* __restrict__ fin_end,
                                                                         const int* __restrict__ lengths, int n_frames, int W, int n_best,
                                                                         int* __restrict__ tokens, int* __restrict__ frames,
                                                                         float* __restrict__ lm_scores) {
  const int n = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const int4* const nodes = nodes_all + (size_t)b * ((size_t)n_frames * W + 1);
  const BeamPieceNode* const nodes_lm = nodes_lm_all + (size_t)b * ((size_t)n_frames * W + 1);
  int* const tok = tokens + ((size_t)b * n_best + n) * n_frames;
  int* const frm = frames + ((size_t)b * n_best + n) * n_frames;
  const int L = min(max(lengths[(size_t)b * n_best + n], 0), n_frames);
  for (int p = L + lane; p < n_frames; p += 64) { tok[p] = 0; frm[p] = 0; }
  if (lane == 0) {
    int id = fin[(size_t)b * BEAM_FIN + n];
    const bool have = id >= 0;
    const int last_id = n_frames * W;
    for (int p = L - 1; p >= 0; --p) {                 // backward: the tokens; the node ids wait in the frames row
      int4 nd = make_int4(0, 0, 0, 0);
      const bool ok = id >= 1 && id <= last_id;
      if (ok) nd = nodes[id];
      tok[p] = nd.y;
      frm[p] = ok ? id : 0;
      id = nd.x;
    }
    double sum = 0.0;
    for (int p = 0; p < L; ++p) {                      // forward: the frames and the LM score
      const int q = frm[p];
      int f = 0;
      if (q >= 1 && q <= last_id) { f = nodes[q].z; sum = sum + nodes_lm[q].log10; }
      frm[p] = f;
    }
    lm_scores[(size_t)b * n_best + n] = have ? (float)(sum + fin_end[(size_t)b * BEAM_FIN + n]) : 0.f;
  }
}

}  // namespace ts

// What ts_ctc_beam_piece_lm_search launches, as a function of the class count and the two widths alone
struct BeamPieceLaunch {
  int cap, cands, threads;
  size_t lds;
};
static int beam_piece_launch_config(int n_classes, int beam_width, int token_cap, BeamPieceLaunch* c) {
  if (n_classes <= 0 || beam_width < 1 || token_cap < 1) return TS_EINVAL;
  if (beam_width > ts::BEAM_MAX || token_cap > ts::BEAM_MAX || n_classes > (1 << 24)) return TS_EUNSUPPORTED;
  c->cap = token_cap < n_classes - 1 ? token_cap : n_classes - 1;
  c->cands = beam_width * (c->cap + 1);
  if (c->cands > ts::BEAM_PIECE_CANDS) return TS_EUNSUPPORTED;
  c->threads = ts::round_up(c->cands, 64);
  c->lds = (size_t)96 * ts::round_up(beam_width, 8) + (size_t)16 * ts::round_up(c->cands, 8) + (size_t)48 * ts::beam_even(c->cap + 2) + 16 + 32 * ts::BEAM_ROW;
  return TS_OK;
}

extern "C" int ts_ctc_beam_piece_lm_abi_version(void) { return TS_CTC_BEAM_PIECE_LM_ABI_VERSION; }

extern "C" int ts_ctc_beam_piece_lm_launch_config(int32_t n_classes, int32_t beam_width, int32_t token_cap, int32_t* threads, int32_t* lds_bytes,
                                                  int32_t* candidates) {
  if (!threads || !lds_bytes || !candidates) return TS_EINVAL;
  BeamPieceLaunch c{};
  const int st = beam_piece_launch_config(n_classes, beam_width, token_cap, &c);
  if (st != TS_OK) return st;
  *threads = c.threads; *lds_bytes = (int32_t)c.lds; *candidates = c.cands;
  return TS_OK;
}

extern "C" int64_t ts_ctc_beam_piece_lm_workspace_bytes(int32_t batch, int32_t n_frames, int32_t beam_width, int32_t token_cap) {
  if (batch <= 0 || n_frames <= 0 || beam_width < 1 || token_cap < 1) return TS_EINVAL;
  if (beam_width > ts::BEAM_MAX || token_cap > ts::BEAM_MAX) return TS_EUNSUPPORTED;
  return (int64_t)batch * (32 * ((int64_t)n_frames * beam_width + 1) + 12 * (int64_t)n_frames * (token_cap + 2) + 8 * ts::BEAM_ROW * (int64_t)n_frames +
                           12 * ts::BEAM_FIN);
}

extern "C" int ts_ctc_beam_piece_lm_search(const float* logits, int32_t batch, int32_t n_classes, int32_t n_frames, int32_t pitch,
                                           const int32_t* input_len, int32_t blank, int32_t beam_width, int32_t token_cap, int32_t n_best,
                                           int32_t score_eos, const ts_ctc_lm* lm, const ts_ctc_lexicon* lexicon, const ts_ctc_pieces* pieces,
                                           int32_t* tokens, int32_t* frames, int32_t* lengths, float* scores, float* lm_scores, int32_t* counts,
                                           void* workspace, void* stream_) {
  using namespace ts;
  if (!logits || !lm || !lexicon || !pieces || !tokens || !frames || !lengths || !scores || !lm_scores || !counts || !workspace) return TS_EINVAL;
  if (batch <= 0 || n_classes <= 0 || n_frames <= 0 || pitch < n_frames) return TS_EINVAL;
  if (blank < 0 || blank >= n_classes) return TS_EINVAL;
  if (n_best < 1) return TS_EINVAL;
  if (!lm->arc_begin || !lm->arc_class || !lm->arc_next || !lm->arc_factor || !lm->arc_log10 || !lm->bo_next || !lm->bo_factor || !lm->bo_log10)
    return TS_EINVAL;
  if (lm->has_eos && (!lm->eos_factor || !lm->eos_log10)) return TS_EINVAL;
  if (lm->n_states < 1 || lm->n_arcs < 0 || lm->start_state < 0 || lm->start_state >= lm->n_states) return TS_EINVAL;
  const ts_ctc_lexicon& lx = *lexicon;                 // (its delimiter is not looked at: a word ends where a word-start piece follows)
  if (lx.n_nodes < 1 || lx.n_edges < 0 || lx.n_words < 0) return TS_EINVAL;
  if (!lx.edge_begin || !lx.node_word || !lx.oov_factor) return TS_EINVAL;
  if (lx.n_edges > 0 && (!lx.edge_class || !lx.edge_next)) return TS_EINVAL;
  if (lx.n_words > 0 && (!lx.word_class || !lx.word_factor)) return TS_EINVAL;
  const ts_ctc_pieces& pc = *pieces;
  if (pc.n_classes != n_classes || pc.n_letters < 0 || pc.n_piece_letters < 0) return TS_EINVAL;
  if (!pc.piece_begin || !pc.piece_kind) return TS_EINVAL;
  if (pc.n_piece_letters > 0 && !pc.piece_letter) return TS_EINVAL;
  BeamPieceLaunch cfg{};
  const int cst = beam_piece_launch_config(n_classes, beam_width, token_cap, &cfg);
  if (cst != TS_OK) return cst;
  if (n_best > BEAM_MAX) return TS_EUNSUPPORTED;
  if (n_best > beam_width) return TS_EINVAL;
  if (misaligned(workspace)) return TS_EUNSUPPORTED;
  if (misaligned(lm->arc_factor, 7) || misaligned(lm->arc_log10, 7) || misaligned(lm->bo_factor, 7) || misaligned(lm->bo_log10, 7) ||
      misaligned(lm->eos_factor, 7) || misaligned(lm->eos_log10, 7) || misaligned(lx.word_factor, 7) || misaligned(lx.oov_factor, 7))
    return TS_EUNSUPPORTED;
  if ((int64_t)n_frames * beam_width + 1 > 0x7fffffff) return TS_EUNSUPPORTED;     // trie node ids are int32
  TS_STREAM;
  // workspace: the two halves of the nodes (16 bytes each), the records' probabilities (8), the class rows (8), the pending-word and </s> scores
  // of the final nodes (8), the records' ids (4), the final nodes (4); laid out for the clamped token_cap, inside the
  // ts_ctc_beam_piece_lm_workspace_bytes of the caller's
  char* ws = static_cast<char*>(workspace);
  const size_t n_nodes = (size_t)batch * ((size_t)n_frames * beam_width + 1);
  BeamPieceArgs a{};
  a.nodes = reinterpret_cast<int4*>(ws);
  ws += n_nodes * sizeof(int4);
  a.nodes_lm = reinterpret_cast<BeamPieceNode*>(ws);
  ws += n_nodes * sizeof(BeamPieceNode);
  double* const cp = reinterpret_cast<double*>(ws);
  ws += (size_t)batch * n_frames * (cfg.cap + 2) * sizeof(double);
  double* const prow = reinterpret_cast<double*>(ws);
  ws += (size_t)batch * n_frames * BEAM_ROW * sizeof(double);
  a.fin_end = reinterpret_cast<double*>(ws);
  ws += (size_t)batch * BEAM_FIN * sizeof(double);
  int* const cid = reinterpret_cast<int*>(ws);
  ws += (size_t)batch * n_frames * (cfg.cap + 2) * sizeof(int);
  a.fin = reinterpret_cast<int*>(ws);
  a.logits = logits; a.input_len = input_len; a.cp = cp; a.cid = cid; a.prow = prow; a.lengths = lengths; a.scores = scores; a.counts = counts;
  a.arc_begin = lm->arc_begin; a.arc_class = lm->arc_class; a.arc_next = lm->arc_next;
  a.arc_factor = static_cast<const double*>(lm->arc_factor); a.arc_log10 = static_cast<const double*>(lm->arc_log10);
  a.bo_next = lm->bo_next; a.bo_factor = static_cast<const double*>(lm->bo_factor); a.bo_log10 = static_cast<const double*>(lm->bo_log10);
  a.eos_factor = static_cast<const double*>(lm->eos_factor); a.eos_log10 = static_cast<const double*>(lm->eos_log10);
  a.edge_begin = lx.edge_begin; a.edge_class = lx.edge_class; a.edge_next = lx.edge_next; a.node_word = lx.node_word; a.word_class = lx.word_class;
  a.word_factor = static_cast<const double*>(lx.word_factor); a.oov_factor = static_cast<const double*>(lx.oov_factor);
  a.piece_begin = pc.piece_begin; a.piece_letter = pc.piece_letter; a.piece_kind = pc.piece_kind;
  a.n_states = lm->n_states; a.n_arcs = lm->n_arcs; a.start_state = lm->start_state; a.eos = (score_eos && lm->has_eos) ? 1 : 0;
  a.n_nodes = lx.n_nodes; a.n_edges = lx.n_edges; a.n_words = lx.n_words; a.unk_class = lx.unk_class;
  a.n_piece_letters = pc.n_piece_letters;
  a.n_classes = n_classes; a.n_frames = n_frames; a.pitch = pitch; a.W = beam_width; a.cap = cfg.cap; a.n_best = n_best; a.S = cfg.cands;
  hipLaunchKernelGGL(ctc_beam_cand_kernel, dim3((unsigned)((n_frames + 3) / 4), (unsigned)batch), dim3(256), 0, stream, logits, n_classes, n_frames,
                     pitch, input_len, blank, cfg.cap, cp, cid, prow);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(ctc_beam_piece_lm_search_kernel, dim3((unsigned)batch), dim3((unsigned)cfg.threads), cfg.lds, stream, a);
  e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(ctc_beam_piece_lm_backtrace_kernel, dim3((unsigned)n_best, (unsigned)batch), dim3(64), 0, stream, a.nodes, a.nodes_lm, a.fin,
                     a.fin_end, lengths, n_frames, beam_width, n_best, tokens, frames, lm_scores);
  return hip_status(hipGetLastError());
}
