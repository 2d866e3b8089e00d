/*
 * thunder_speech_amd/ctc_beam_piece_lm.h -- companion C ABI of include/thunder_speech_amd.h: CTC prefix beam search over a SENTENCEPIECE vocabulary
 * with shallow fusion of a WORD-level n-gram language model, a lexicon and hot-word boosting (csrc/ctc_beam_piece_lm.hip).  The acoustic model's
 * CTC classes are pieces: a piece spells zero or more LETTERS, and a piece that begins with U+2581 starts a word.  thunder_speech_amd/ctc_lm.py
 * (PieceWordNGramLM) reads a word-level ARPA file and compiles the tables this header takes.  The same shared library exports these entry
 * points; the conventions are the core header's (DEVICE pointers into caller-owned buffers, `stream` a hipStream_t passed as void*, 0 / TS_EINVAL /
 * TS_EUNSUPPORTED / positive hipError_t returns, nothing allocates, frees or synchronises, so every call can be captured into a hipGraph).  The
 * core ABI, ctc_beam_word_lm.h and the other companions are unchanged by this header; it is versioned on its own by
 * TS_CTC_BEAM_PIECE_LM_ABI_VERSION.
 *
 * No reference call site: the reference decodes greedily only.  Input: logits [B][V][pitch] f32 BEFORE softmax, time contiguous.
 *
 * THE WORD AUTOMATON is the ts_ctc_lm of ctc_beam_word_lm.h, unchanged: word ids as classes, unk_class for <unk>-as-a-word.
 *
 * THE LEXICON is the ts_ctc_lexicon of ctc_beam_word_lm.h with two differences: edge_class holds LETTER IDS (0 <= id < n_letters), not CTC
 * classes, and `delimiter` is ignored (the host sets it to -1; it is not validated here).  Every segmentation of a word into pieces walks the
 * same letters and so reaches the same node.
 *
 * THE PIECES (ts_ctc_pieces) say what a CTC class spells: piece_letter[piece_begin[c] .. piece_begin[c + 1]) are the letters of class c in order
 * (none for a bare U+2581 piece, for the blank and for a class of kind 2), and piece_kind[c] is 0 for a piece that continues a word, 1 for a
 * piece that starts one, 2 for a class without a spelling (a special token, or a piece that cannot be split into the letters).  Every index read
 * from a table is clamped to its table before it is used, so inconsistent tables give wrong scores, never a read outside them.
 *
 * THE ALGORITHM is ts_ctc_beam_word_lm_search as ctc_beam_word_lm.h specifies it -- the same candidate pre-pass, every child of every slot
 * ranked, linear f64 masses rescaled per frame by the exact power of two, merges through one slot per beam entry, no atomics, no exp and no log
 * of the LM on the device; a beam entry carries (word state s, lexicon state x), x = 0 the root, x > 0 a trie node, x = -1 outside the lexicon;
 * prefixes are sequences of CLASSES, so two segmentations of one text are two prefixes -- with the child rule replaced.  A child for a class c
 * (not the blank) of an entry (s, x) does, in this order, one f64 rounding per product:
 *   1. Word end, if piece_kind[c] == 1 and x != 0: the pending word ends exactly as at the delimiter of ctc_beam_word_lm.h -- the lookup of
 *      word_class[node_word[x]] (unk_class without a word) from s, then word_factor[w] or, for a node x > 0 that is not terminal,
 *      oov_factor[0]; s' = the arc's target, x = 0; the node's log10 is the lookup's log10.  With piece_kind[c] == 1 and x == 0 nothing happens
 *      (the start of a clip, or the step after a bare U+2581 piece).
 *   2. Letters, for each letter of the piece in order: x >= 0 and node x has an edge of that letter: x = its edge_next;  x >= 0 and it has none:
 *      x = -1 and mass = mass oov_factor[0];  x = -1: it stays -1.
 *   3. No spelling, piece_kind[c] == 2: one letter that no node has an edge for -- from x >= 0 to x = -1, paying oov_factor[0]; from x = -1
 *      nothing changes.  It never ends a word.
 *   A class of kind 0 or 2 leaves s alone and its node's log10 is 0.  After the last frame the pending word and </s> are handled exactly as in
 *   ctc_beam_word_lm.h.
 *   SUPPORTED: beam_width <= 64, token_cap <= 64 and beam_width (cap + 1) <= 1024, as there.
 *   Outputs: those of ts_ctc_beam_word_lm_search.
 *
 * Next steps, NOT in this ABI: merging hypotheses whose different segmentations spell one text; LM look-ahead inside a word; boosting of partial
 * hot-word matches; neural LMs; candidate sets beyond 1024.
 */
#ifndef THUNDER_SPEECH_AMD_CTC_BEAM_PIECE_LM_H
#define THUNDER_SPEECH_AMD_CTC_BEAM_PIECE_LM_H

#include <stdint.h>

#include "thunder_speech_amd/ctc_beam_word_lm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS_CTC_BEAM_PIECE_LM_ABI_VERSION 1

/* What the CTC classes spell: a HOST struct of DEVICE pointers. */
typedef struct ts_ctc_pieces {
  int32_t n_classes, n_letters, n_piece_letters;
  const int32_t* piece_begin;    /* [n_classes + 1] into piece_letter */
  const int32_t* piece_letter;   /* [n_piece_letters] letter ids, 0 <= id < n_letters */
  const int32_t* piece_kind;     /* [n_classes] 0 continues a word, 1 starts a word, 2 has no spelling */
} ts_ctc_pieces;

/* Version of this companion ABI (a binder checks it next to ts_abi_version). */
int ts_ctc_beam_piece_lm_abi_version(void);

/* Host only: what the search kernel of ts_ctc_beam_piece_lm_search launches: the values and the refusals of ts_ctc_beam_word_lm_launch_config.
 *   candidates  beam_width (cap + 1), cap = min(token_cap, n_classes - 1)
 *   threads     round_up(candidates, 64)
 *   lds_bytes   96 round_up(beam_width, 8) + 16 round_up(candidates, 8) + 48 round_up(cap + 2, 2) + 2064 */
int ts_ctc_beam_piece_lm_launch_config(int32_t n_classes, int32_t beam_width, int32_t token_cap, int32_t* threads, int32_t* lds_bytes,
                                       int32_t* candidates);

/* Bytes of workspace ts_ctc_beam_piece_lm_search needs: batch (32 (n_frames beam_width + 1) + 12 n_frames (token_cap + 2) + 512 n_frames + 768),
 * the layout of ts_ctc_beam_word_lm_workspace_bytes, or TS_EINVAL (< 0) for batch <= 0, n_frames <= 0, beam_width < 1 or token_cap < 1,
 * TS_EUNSUPPORTED for beam_width or token_cap > 64. */
int64_t ts_ctc_beam_piece_lm_workspace_bytes(int32_t batch, int32_t n_frames, int32_t beam_width, int32_t token_cap);

/* The fused search as specified above, in three launches on `stream`: the frame candidates of ts_ctc_beam_search, the search with one workgroup
 * per utterance, and the backtrace of the n_best final trie nodes.  The arguments and the outputs are those of ts_ctc_beam_word_lm_search, plus
 * the pieces.
 * workspace: ts_ctc_beam_piece_lm_workspace_bytes bytes, 16-byte aligned; contents are scratch.
 * TS_EINVAL: what ts_ctc_beam_word_lm_search refuses with it, except that lexicon->delimiter is not looked at; a NULL pieces, piece_begin or
 * piece_kind; a NULL piece_letter with n_piece_letters > 0; pieces->n_classes != n_classes; n_letters < 0 or n_piece_letters < 0.
 * TS_EUNSUPPORTED: what ts_ctc_beam_word_lm_search refuses with it. */
int ts_ctc_beam_piece_lm_search(const float* logits, int32_t batch, int32_t n_classes, int32_t n_frames, int32_t pitch, const int32_t* input_len,
                                int32_t blank, int32_t beam_width, int32_t token_cap, int32_t n_best, int32_t score_eos, const ts_ctc_lm* lm,
                                const ts_ctc_lexicon* lexicon, const ts_ctc_pieces* pieces, int32_t* tokens, int32_t* frames, int32_t* lengths,
                                float* scores, float* lm_scores, int32_t* counts, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* THUNDER_SPEECH_AMD_CTC_BEAM_PIECE_LM_H */
