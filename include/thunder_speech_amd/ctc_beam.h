/*
 * thunder_speech_amd/ctc_beam.h -- companion C ABI of include/thunder_speech_amd.h: CTC prefix beam search with n-best output
 * (csrc/ctc_beam.hip).  Where ts_greedy_decode follows one path, this decoder sums the probability of all alignments of a transcript and returns
 * the n best transcripts with their CTC scores.  The same shared library exports these entry points; the conventions are the core header's
 * (DEVICE pointers into caller-owned buffers, `stream` a hipStream_t passed as void*, 0 / TS_EINVAL / TS_EUNSUPPORTED / positive hipError_t
 * returns, nothing allocates, frees or synchronises, so every call can be captured into a hipGraph).  The core ABI (TS_ABI_VERSION) and the other
 * companions are unchanged by this header; it is versioned on its own by TS_CTC_BEAM_ABI_VERSION.
 *
 * No reference call site: the reference decodes greedily only (module.py:98-101).  Input: logits [B][V][pitch] f32 BEFORE softmax, time contiguous.
 *
 * THE ALGORITHM, per utterance over the frames t < T, T = clamp(input_len[b], 0, n_frames) (n_frames when input_len is NULL):
 *   Frame candidates: the blank, always, and the token_cap non-blank classes with the largest raw f32 logit of the frame (the lowest class index
 *     wins ties; selection on raw logits equals selection on probabilities and is exact).  p[c] = exp(x[c] - max x) / sum exp(x - max x) in f64.
 *   Beam: at most beam_width distinct prefixes, each with p_b (mass of its alignments ending in blank), p_nb (mass ending in its last token) and
 *     a trie node.  It starts with the empty prefix, p_b = 1, p_nb = 0.
 *   Step of beam entry i, tot = p_b + p_nb:
 *     stay (same prefix):       p_b' = tot p[blank];  p_nb' = p_nb p[last_i] (0 for the empty prefix; applied whether or not last_i is a candidate)
 *     child for candidate c:    p_nb' = (c == last_i ? p_b : tot) p[c];  p_b' = 0
 *     merge: a child whose prefix is already in the beam as entry j adds its mass to j's stay p_nb' and is no candidate of its own.  Prefixes are
 *       identified by their length and a 64-bit hash of the token string: h(empty) = 0, h(s + c) = mix(h(s) + 0x9E3779B97F4A7C15 (c + 1)) with
 *       mix the splitmix64 finaliser (z ^= z >> 30, z *= 0xBF58476D1CE4E5B9, z ^= z >> 27, z *= 0x94D049BB133111EB, z ^= z >> 31).  (Node ids are
 *       not compared: a prefix can stay in the beam while its parent drops out and re-enters under a new node.)
 *     candidates with key 0 are dropped.
 *   Selection: key = p_b' + p_nb'; the beam_width largest keys are kept; equal keys fall in candidate order (stay candidates first, by beam slot,
 *     then children by (parent slot, class index)).  The new beam is stored in rank order (slot = rank).  A kept child gets a new trie node
 *     (parent node, token, frame t) in the workspace; nodes are never reused.
 *   Arithmetic: p_b and p_nb are linear-domain f64, rescaled once per frame by the exact power of two 2^-ilogb(largest key); the exponents are
 *     summed as integers.  No exp and no log sits in the frame-to-frame dependency chain.  A candidate that underflows against the best of its
 *     frame is 0 and is dropped.  score = log(key) + exponent_sum ln 2 in f64, rounded to f32 once.  No atomics: equal arguments give equal bits.
 *
 * Next steps, NOT in this ABI: language-model fusion (n-gram or neural), lexicon constraints, word-insertion bonuses, beams wider than 64,
 * word-level timestamps of beam hypotheses (run ts_ctc_align on the chosen text for those).
 */
#ifndef THUNDER_SPEECH_AMD_CTC_BEAM_H
#define THUNDER_SPEECH_AMD_CTC_BEAM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TS_CTC_BEAM_ABI_VERSION 1

/* Version of this companion ABI (a binder checks it next to ts_abi_version). */
int ts_ctc_beam_abi_version(void);

/* Host only: what the search kernel of ts_ctc_beam_search launches.  cap = min(token_cap, n_classes - 1).
 *   candidates  ranked candidates per frame: beam_width stay candidates, every child of beam slot 0, and of slot i >= 1 its children of the
 *               min(cap, ceil(beam_width / i)) most probable classes.  (The beam is stored in rank order, so the child of slot i and the r-th most
 *               probable class is beaten by the i r children of lower slots and at-least-as-probable classes that are not those slots' `c == last`
 *               child, or by the stay candidates these merged into: with i r >= beam_width it cannot be kept and is never formed.)
 *   threads     round_up(candidates, 64): the workgroup, one thread per ranked candidate
 *   lds_bytes   dynamic LDS of the launch: 88 round_up(beam_width, 8) + 16 round_up(candidates, 8) + 48 round_up(cap + 2, 2) + 2064
 * TS_EINVAL: a NULL pointer, n_classes <= 0, beam_width < 1, token_cap < 1.  TS_EUNSUPPORTED: beam_width or token_cap > 64, n_classes > 2^24. */
int ts_ctc_beam_launch_config(int32_t n_classes, int32_t beam_width, int32_t token_cap, int32_t* threads, int32_t* lds_bytes, int32_t* candidates);

/* Bytes of workspace ts_ctc_beam_search needs: batch (16 (n_frames beam_width + 1) + 12 n_frames (token_cap + 2) + 512 n_frames + 256) -- the
 * trie nodes (16 bytes each), the frame records, the per-class probabilities of a frame (up to 64 classes) and the final nodes -- or TS_EINVAL (< 0) for batch <= 0, n_frames <= 0, beam_width < 1 or token_cap < 1,
 * TS_EUNSUPPORTED for beam_width or token_cap > 64. */
int64_t ts_ctc_beam_workspace_bytes(int32_t batch, int32_t n_frames, int32_t beam_width, int32_t token_cap);

/* CTC prefix beam search as specified above, in three launches on `stream`: the frame candidates in parallel over batch x frames (per frame
 * cap + 1 (class id, f64 probability) records -- the blank, then the kept classes by descending logit, the lowest class first among equals --
 * and the frame's normaliser), the search with one workgroup per utterance, and the backtrace of the n_best final trie nodes.
 *   tokens   int32 [B][n_best][n_frames]   class ids of hypothesis n, in forward order
 *   frames   int32 [B][n_best][n_frames]   the frame at which each token's trie node was created
 *   lengths  int32 [B][n_best]
 *   scores   f32 [B][n_best]               log of the summed probability of all alignments of the hypothesis that survived the pruning
 *   counts   int32 [B]                     hypotheses actually produced (<= n_best), best first
 * Entries beyond a length or a count are zero; scores beyond the count are -inf.  T = 0 gives one hypothesis: the empty string with score 0.
 * input_len may be NULL.  Logits at t >= T are not read.  token_cap is clamped to n_classes - 1.
 * workspace: ts_ctc_beam_workspace_bytes bytes, 16-byte aligned; contents are scratch.
 * TS_EINVAL: a NULL pointer (input_len and the stream excepted), batch <= 0, n_classes <= 0, n_frames <= 0, pitch < n_frames, blank outside
 * [0, n_classes), beam_width, token_cap or n_best < 1, n_best > beam_width.  TS_EUNSUPPORTED: beam_width, token_cap or n_best > 64 (checked
 * before n_best > beam_width), n_classes > 2^24, workspace not 16-byte aligned. */
int ts_ctc_beam_search(const float* logits, int32_t batch, int32_t n_classes, int32_t n_frames, int32_t pitch, const int32_t* input_len,
                       int32_t blank, int32_t beam_width, int32_t token_cap, int32_t n_best, int32_t* tokens, int32_t* frames, int32_t* lengths,
                       float* scores, int32_t* counts, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* THUNDER_SPEECH_AMD_CTC_BEAM_H */
