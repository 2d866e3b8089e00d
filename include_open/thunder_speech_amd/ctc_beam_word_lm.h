/*
 * thunder_speech_amd/ctc_beam_word_lm.h -- companion C ABI of include/thunder_speech_amd.h: CTC prefix beam search over a CHARACTER vocabulary with
 * shallow fusion of a WORD-level n-gram language model, a lexicon and hot-word boosting (csrc/ctc_beam_word_lm.hip).  The acoustic model's CTC
 * classes are letters and one word delimiter; the LM's words are spelled in those letters.  thunder_speech_amd/ctc_lm.py (WordNGramLM) reads a
 * word-level ARPA file and compiles the tables this header takes.  The same shared library exports these entry points; the conventions are the
 * core header's (DEVICE pointers into caller-owned buffers, `stream` a hipStream_t passed as void*, 0 / TS_EINVAL / TS_EUNSUPPORTED / positive
 * hipError_t returns, nothing allocates, frees or synchronises, so every call can be captured into a hipGraph).  The core ABI, ctc_beam.h,
 * ctc_beam_lm.h and the other companions are unchanged by this header; it is versioned on its own by TS_CTC_BEAM_WORD_LM_ABI_VERSION.
 *
 * No reference call site: the reference decodes greedily only.  Input: logits [B][V][pitch] f32 BEFORE softmax, time contiguous.
 *
 * THE WORD AUTOMATON is a ts_ctc_lm (ctc_beam_lm.h) whose classes are WORD IDS, with one extra class, unk_class, for <unk>-as-a-word: that class
 * takes <unk>'s unigram or the floor and leads to state 0, so state 0's arcs are the whole unigram table.  Its lookup is the lookup of
 * ctc_beam_lm.h, unchanged: back-off arcs, then the arc, one f64 product each; a class that state 0 lacks has factor 0.
 *
 * THE LEXICON is a trie over the letter classes.  Node 0 is the root; node x has edges edge_begin[x] <= e < edge_begin[x + 1], sorted by class with
 * no class twice: (edge_class, edge_next).  node_word[x] is the word that ends at node x (the node is then TERMINAL), or -1.  Word w has the
 * word-automaton class word_class[w] (unk_class for a word the LM lacks) and the hot-word factor word_factor[w] (f64, e^boost formed on the host;
 * 1 for a word that is not hot).  oov_factor[0] (f64, e^oov_score) is what a word outside the lexicon pays, once.  Every index read from a table
 * is clamped to its table before it is used, so inconsistent tables give wrong scores, never a read outside them.
 *
 * THE ALGORITHM is ts_ctc_beam_lm_search as specified in ctc_beam_lm.h -- the frame candidates of ctc_beam.h, every child of every beam slot
 * ranked (beam_width (cap + 1) candidates, a thread per candidate), linear f64 masses rescaled per frame by the exact power of two, merges through
 * one slot per beam entry, counting rank, trie nodes, no exp and no log of the LM on the device, no atomics -- with these changes:
 *   State: a beam entry carries the word automaton's state s and a lexicon state x: x = 0 the root of the trie, x > 0 a trie node, x = -1 "outside
 *     the lexicon".  The empty prefix starts in (start_state, 0).  Both are functions of the prefix alone, so alignments that merge agree on them.
 *   Child of an entry (s, x) for a class c that is neither the blank nor `delimiter`: s is unchanged, the node's log10 is 0, and
 *       x >= 0 and node x has an edge of class c:   x' = that edge's edge_next, factor 1
 *       x >= 0 and node x has no such edge:         x' = -1, mass = mass oov_factor[0]
 *       x = -1:                                     x' = -1, factor 1
 *   Child for c == delimiter:
 *       x == 0 (an empty word: a leading or doubled delimiter): (s, 0) unchanged, factor 1, log10 0.
 *       Otherwise the word is w = node_word[x], defined when x > 0 and the node is terminal.
 *         With a word:    the lookup of class word_class[w] from s (the bo_factor met, in the order met, then the arc_factor: one f64 rounding
 *                         each), then mass = mass word_factor[w].
 *         Without one (x = -1, or a node that is not terminal): the lookup of class unk_class from s; then, when x > 0, mass = mass oov_factor[0]
 *                         -- a word that left the trie paid when it left, so every out-of-lexicon word pays the factor exactly once.
 *         x' = 0, s' = the arc's arc_next.  The node's log10 is the unweighted log10 met on the lookup (bo_log10 in the order met, then arc_log10,
 *         summed in f64 from 0).  Neither word_factor nor oov_factor enters lm_scores.
 *   After the last frame, before the final ranking: an entry with x != 0 takes the factors of its pending word exactly as if a delimiter followed
 *     (whatever score_eos says), which also gives the state s' that </s> is scored from; then its key takes eos_factor[s'] under the score_eos /
 *     has_eos rule of ctc_beam_lm.h.  The pending word's log10 is added to the hypothesis' lm_score next to the </s> term (pending + </s>, summed
 *     in f64 from 0, then added to the sum over the trie nodes).  T = 0 gives the empty hypothesis (x = 0: no pending word), with </s> as there.
 *   SUPPORTED: beam_width <= 64, token_cap <= 64 and beam_width (cap + 1) <= 1024, as in ctc_beam_lm.h.
 *   Outputs: those of ts_ctc_beam_lm_search.
 *
 * Next steps, NOT in this ABI: sentencepiece vocabularies, where a word starts at a U+2581 piece (those have ctc_beam_piece_lm.h, which reuses the
 * structs of this header); LM look-ahead inside a word; boosting of partial hot-word matches; neural LMs (rescore the n-best list on the host for those); candidate sets
 * beyond 1024.
 */
#ifndef THUNDER_SPEECH_AMD_CTC_BEAM_WORD_LM_H
#define THUNDER_SPEECH_AMD_CTC_BEAM_WORD_LM_H

#include <stdint.h>

#include "thunder_speech_amd/ctc_beam_lm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS_CTC_BEAM_WORD_LM_ABI_VERSION 1

/* The lexicon of one (oov_score, boosts) setting: a HOST struct of DEVICE pointers.
 *   edge_begin [n_nodes + 1], edge_class / edge_next [n_edges] (sorted by class per node), node_word [n_nodes] (-1 = not a word),
 *   word_class [n_words], word_factor f64 [n_words], oov_factor f64 [1] (a table of one element, so that a new setting is a write at a fixed
 *   address).  delimiter: the CTC class that ends a word.  unk_class: the word automaton's class of <unk>-as-a-word. */
typedef struct ts_ctc_lexicon {
  int32_t n_nodes, n_edges, n_words, delimiter, unk_class;
  const int32_t* edge_begin;
  const int32_t* edge_class;
  const int32_t* edge_next;
  const int32_t* node_word;
  const int32_t* word_class;
  const void* word_factor;
  const void* oov_factor;
} ts_ctc_lexicon;

/* Version of this companion ABI (a binder checks it next to ts_abi_version). */
int ts_ctc_beam_word_lm_abi_version(void);

/* Host only: what the search kernel of ts_ctc_beam_word_lm_search launches.  cap = min(token_cap, n_classes - 1).
 *   candidates  beam_width (cap + 1): the stay candidates, then every child of every slot
 *   threads     round_up(candidates, 64): the workgroup, one thread per candidate
 *   lds_bytes   dynamic LDS of the launch: 96 round_up(beam_width, 8) + 16 round_up(candidates, 8) + 48 round_up(cap + 2, 2) + 2064
 * TS_EINVAL: a NULL pointer, n_classes <= 0, beam_width < 1, token_cap < 1.  TS_EUNSUPPORTED: beam_width or token_cap > 64, n_classes > 2^24,
 * candidates > 1024. */
int ts_ctc_beam_word_lm_launch_config(int32_t n_classes, int32_t beam_width, int32_t token_cap, int32_t* threads, int32_t* lds_bytes,
                                      int32_t* candidates);

/* Bytes of workspace ts_ctc_beam_word_lm_search needs: batch (32 (n_frames beam_width + 1) + 12 n_frames (token_cap + 2) + 512 n_frames + 768) --
 * the trie nodes (32 bytes each: parent, token, frame, depth; the token's log10, the word state and the lexicon state entered), the frame records,
 * the per-class probabilities of a frame (up to 64 classes), the final nodes and their pending-word and </s> scores -- or TS_EINVAL (< 0) for
 * batch <= 0, n_frames <= 0, beam_width < 1 or token_cap < 1, TS_EUNSUPPORTED for beam_width or token_cap > 64. */
int64_t ts_ctc_beam_word_lm_workspace_bytes(int32_t batch, int32_t n_frames, int32_t beam_width, int32_t token_cap);

/* The fused search as specified above, in three launches on `stream`: the frame candidates of ts_ctc_beam_search, the search with one workgroup
 * per utterance, and the backtrace of the n_best final trie nodes.  The arguments and the outputs are those of ts_ctc_beam_lm_search (tokens,
 * frames int32 [B][n_best][n_frames], lengths int32 [B][n_best], scores, lm_scores f32 [B][n_best], counts int32 [B]; entries beyond a length or a
 * count are zero, scores beyond the count are -inf), plus the lexicon.  `lm` is the word automaton.
 * workspace: ts_ctc_beam_word_lm_workspace_bytes bytes, 16-byte aligned; contents are scratch.
 * TS_EINVAL: what ts_ctc_beam_lm_search refuses with it; a NULL lexicon, edge_begin, node_word or oov_factor; a NULL edge_class or edge_next with
 * n_edges > 0; a NULL word_class or word_factor with n_words > 0; n_nodes < 1, n_edges < 0, n_words < 0; delimiter outside [0, n_classes) or
 * equal to blank.  TS_EUNSUPPORTED: what ts_ctc_beam_lm_search refuses with it; word_factor or oov_factor not 8-byte aligned. */
int ts_ctc_beam_word_lm_search(const float* logits, int32_t batch, int32_t n_classes, int32_t n_frames, int32_t pitch, const int32_t* input_len,
                               int32_t blank, int32_t beam_width, int32_t token_cap, int32_t n_best, int32_t score_eos, const ts_ctc_lm* lm,
                               const ts_ctc_lexicon* lexicon, int32_t* tokens, int32_t* frames, int32_t* lengths, float* scores, float* lm_scores,
                               int32_t* counts, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* THUNDER_SPEECH_AMD_CTC_BEAM_WORD_LM_H */
