/*
 * thunder_speech_amd/ctc_beam_lm.h -- companion C ABI of include/thunder_speech_amd.h: CTC prefix beam search with shallow fusion of a
 * token-level n-gram language model (csrc/ctc_beam_lm.hip).  The LM's words are the acoustic model's CTC classes (characters, or sentencepiece
 * pieces); thunder_speech_amd/ctc_lm.py reads an ARPA file and compiles the tables this header takes.  The same shared library exports these
 * entry points; the conventions are the core header's (DEVICE pointers into caller-owned buffers, `stream` a hipStream_t passed as void*,
 * 0 / TS_EINVAL / TS_EUNSUPPORTED / positive hipError_t returns, nothing allocates, frees or synchronises, so every call can be captured into a
 * hipGraph).  The core ABI (TS_ABI_VERSION), ctc_beam.h and the other companions are unchanged by this header; it is versioned on its own by
 * TS_CTC_BEAM_LM_ABI_VERSION.
 *
 * No reference call site: the reference decodes greedily only.  Input: logits [B][V][pitch] f32 BEFORE softmax, time contiguous.
 *
 * THE LANGUAGE MODEL: a back-off automaton.  State 0 is the empty context; state s has arcs arc_begin[s] <= a < arc_begin[s + 1], sorted by class
 * with no class twice, and a back-off arc.  Arc a: (arc_class, arc_next, arc_factor, arc_log10); back-off arc of s > 0: (bo_next, bo_factor,
 * bo_log10).  The factors are f64 LINEAR weights formed on the host (ctc_lm.py: arc_factor = 10^(alpha log10 p) e^beta, bo_factor =
 * 10^(alpha log10 bo), eos_factor = 10^(alpha log10 P(</s> | state)), no beta): the device takes no exp and no log of the LM, and every run sees
 * the same doubles.  The *_log10 tables are the unweighted log10 values, for reporting only.
 *   Lookup of class c in state s:   while s has no arc of class c and s != 0: apply (bo_factor[s], bo_log10[s]); s = bo_next[s].
 *                                   Then apply the arc's (arc_factor, arc_log10); the state entered is its arc_next.
 *   State 0 must have an arc for every class but the blank (ctc_lm.py gives a class without a unigram the <unk> unigram, or a floor, with
 *   arc_next 0).  A class that state 0 lacks all the same has factor 0: the child is dropped.  Every index read from a table is clamped to its
 *   table before it is used, so inconsistent tables give wrong scores, never a read outside them.
 *
 * THE ALGORITHM is that of ctc_beam.h (frame candidates, beam of at most beam_width prefixes with p_b / p_nb and a trie node, prefixes identified
 * by length and the 64-bit hash given there, selection of the beam_width largest keys, linear f64 masses rescaled per frame by the exact power of
 * two 2^-ilogb(largest key), no exp and no log in the frame chain, no atomics) with these changes:
 *   State: a beam entry also carries the LM state of its prefix; the empty prefix starts in start_state.
 *   Masses: p_b and p_nb are the acoustic masses TIMES the LM factor of the prefix (the product of the factors met on its tokens' lookups).  The
 *     factor depends on the prefix alone, so alignments that merge agree on it.
 *       stay (same prefix):     p_b' = tot p[blank];  p_nb' = p_nb p[last] + (the mass of the child that merges into this entry, if any)
 *       child for candidate c:  mass = (c == last ? p_b : tot) p[c], then times every bo_factor met on the lookup of c in the entry's state, in
 *                               the order met, then times the arc_factor: one f64 rounding each, no contraction, no reassociation.
 *                               p_nb' = mass, p_b' = 0; a child whose prefix is in the beam already gives its mass to that entry (above).
 *   Candidates: every child of every beam slot is ranked: beam_width (cap + 1) candidates, cap = min(token_cap, n_classes - 1) -- the pruning
 *     of ctc_beam.h needs a child's key to be monotone in (slot, class rank), which a per-(state, class) factor breaks.  Equal keys fall in
 *     candidate order: stay candidates first, by beam slot, then children by (parent slot, class index).  Candidates with key 0 are dropped.
 *     SUPPORTED: beam_width <= 64, token_cap <= 64 and beam_width (cap + 1) <= 1024 (one workgroup, a thread per candidate); TS_EUNSUPPORTED beyond.
 *   Trie nodes also record the LM state entered and the log10 LM score of their token: the bo_log10 met, in the order met, then the arc_log10,
 *     summed in f64 from 0.
 *   After the last frame, with score_eos != 0 and an LM that has </s> (has_eos): each entry's key p_b + p_nb is multiplied by eos_factor[state]
 *     and the final beam is ranked again (equal keys by the rank they had).  T = 0 gives the empty hypothesis, with that factor too.
 *   Outputs: those of ts_ctc_beam_search; `scores` is the log of the fused mass (log(key) + exponent_sum ln 2 in f64, rounded to f32 once); and
 *     lm_scores f32 [B][n_best]: the unweighted log10 LM score of the hypothesis -- the sum over its trie nodes in forward order, in f64 from 0,
 *     plus eos_log10[state] where </s> was applied, rounded to f32 once.  The backtrace kernel forms it.
 *
 * Next steps, NOT in this ABI: word-level LMs over character vocabularies (the LM state would have to wait for a word boundary),
 * lexicon constraints, hot-word boosting, neural LMs (rescore the n-best list on the host for those), candidate sets beyond 1024.
 */
#ifndef THUNDER_SPEECH_AMD_CTC_BEAM_LM_H
#define THUNDER_SPEECH_AMD_CTC_BEAM_LM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TS_CTC_BEAM_LM_ABI_VERSION 1

/* The LM tables of one (alpha, beta) setting: a HOST struct of DEVICE pointers.  The factor and log10 tables hold f64.
 *   arc_begin [n_states + 1], arc_class / arc_next / arc_factor / arc_log10 [n_arcs], bo_next / bo_factor / bo_log10 [n_states] (entry 0 unused),
 *   eos_factor / eos_log10 [n_states] (read only with has_eos != 0). */
typedef struct ts_ctc_lm {
  int32_t n_states, n_arcs, start_state, has_eos;
  const int32_t* arc_begin;
  const int32_t* arc_class;
  const int32_t* arc_next;
  const void* arc_factor;
  const void* arc_log10;
  const int32_t* bo_next;
  const void* bo_factor;
  const void* bo_log10;
  const void* eos_factor;
  const void* eos_log10;
} ts_ctc_lm;

/* Version of this companion ABI (a binder checks it next to ts_abi_version). */
int ts_ctc_beam_lm_abi_version(void);

/* Host only: what the search kernel of ts_ctc_beam_lm_search launches.  cap = min(token_cap, n_classes - 1).
 *   candidates  beam_width (cap + 1): the stay candidates, then every child of every slot
 *   threads     round_up(candidates, 64): the workgroup, one thread per candidate
 *   lds_bytes   dynamic LDS of the launch: 88 round_up(beam_width, 8) + 16 round_up(candidates, 8) + 48 round_up(cap + 2, 2) + 2064
 * TS_EINVAL: a NULL pointer, n_classes <= 0, beam_width < 1, token_cap < 1.  TS_EUNSUPPORTED: beam_width or token_cap > 64, n_classes > 2^24,
 * candidates > 1024. */
int ts_ctc_beam_lm_launch_config(int32_t n_classes, int32_t beam_width, int32_t token_cap, int32_t* threads, int32_t* lds_bytes, int32_t* candidates);

/* Bytes of workspace ts_ctc_beam_lm_search needs: batch (32 (n_frames beam_width + 1) + 12 n_frames (token_cap + 2) + 512 n_frames + 768) -- the
 * trie nodes (32 bytes each), the frame records, the per-class probabilities of a frame (up to 64 classes), the final nodes and their </s>
 * scores -- or TS_EINVAL (< 0) for batch <= 0, n_frames <= 0, beam_width < 1 or token_cap < 1, TS_EUNSUPPORTED for beam_width or token_cap > 64. */
int64_t ts_ctc_beam_lm_workspace_bytes(int32_t batch, int32_t n_frames, int32_t beam_width, int32_t token_cap);

/* The fused search as specified above, in three launches on `stream`: the frame candidates of ts_ctc_beam_search, the search with one workgroup
 * per utterance, and the backtrace of the n_best final trie nodes.
 *   tokens     int32 [B][n_best][n_frames]   class ids of hypothesis n, in forward order
 *   frames     int32 [B][n_best][n_frames]   the frame at which each token's trie node was created
 *   lengths    int32 [B][n_best]
 *   scores     f32 [B][n_best]               log of the fused mass of the hypothesis
 *   lm_scores  f32 [B][n_best]               unweighted log10 LM score of the hypothesis
 *   counts     int32 [B]                     hypotheses actually produced (<= n_best), best first
 * Entries beyond a length or a count are zero; scores beyond the count are -inf (lm_scores there are 0).  input_len may be NULL.  Logits at
 * t >= T are not read.  token_cap is clamped to n_classes - 1.  score_eos is ignored when lm->has_eos is 0.
 * workspace: ts_ctc_beam_lm_workspace_bytes bytes, 16-byte aligned; contents are scratch.
 * TS_EINVAL: a NULL pointer (input_len and the stream excepted; eos_factor and eos_log10 only with has_eos != 0), batch <= 0, n_classes <= 0,
 * n_frames <= 0, pitch < n_frames, blank outside [0, n_classes), beam_width, token_cap or n_best < 1, n_best > beam_width, n_states < 1,
 * n_arcs < 0, start_state outside [0, n_states).  TS_EUNSUPPORTED: beam_width, token_cap or n_best > 64 (checked before n_best > beam_width),
 * n_classes > 2^24, beam_width (min(token_cap, n_classes - 1) + 1) > 1024, workspace or an f64 table not 16-byte / 8-byte aligned. */
int ts_ctc_beam_lm_search(const float* logits, int32_t batch, int32_t n_classes, int32_t n_frames, int32_t pitch, const int32_t* input_len,
                          int32_t blank, int32_t beam_width, int32_t token_cap, int32_t n_best, int32_t score_eos, const ts_ctc_lm* lm,
                          int32_t* tokens, int32_t* frames, int32_t* lengths, float* scores, float* lm_scores, int32_t* counts, void* workspace,
                          void* stream);

#ifdef __cplusplus
}
#endif

#endif /* THUNDER_SPEECH_AMD_CTC_BEAM_LM_H */
