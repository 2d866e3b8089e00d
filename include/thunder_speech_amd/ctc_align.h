/*
 * thunder_speech_amd/ctc_align.h -- companion C ABI of include/thunder_speech_amd.h: "when was it said".  CTC forced alignment of a known
 * transcript (a Viterbi recursion over the blank-extended target) and the frame spans of the greedy transcript (csrc/ctc_align.hip).  The same
 * shared library exports these entry points; the conventions are the core header's (DEVICE pointers into caller-owned buffers, `stream` a
 * hipStream_t passed as void*, 0 / TS_EINVAL / TS_EUNSUPPORTED / positive hipError_t returns, nothing allocates, frees or synchronises, so every
 * call can be captured into a hipGraph).  The core ABI (TS_ABI_VERSION) and the other companions are unchanged by this header; it is versioned on
 * its own by TS_CTC_ALIGN_ABI_VERSION.
 *
 * No reference call site: the reference answers "what was said" only (module.py:98-101 returns bare strings).  The inputs are the ones
 * ts_ctc_loss takes: logits [B][V][pitch] f32 BEFORE softmax, time contiguous, and the int32 targets / lengths ts_ctc_prepare writes.
 */
#ifndef THUNDER_SPEECH_AMD_CTC_ALIGN_H
#define THUNDER_SPEECH_AMD_CTC_ALIGN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TS_CTC_ALIGN_ABI_VERSION 1

/* Version of this companion ABI (a binder checks it next to ts_abi_version). */
int ts_ctc_align_abi_version(void);

/* Host only: what ts_ctc_align launches for a tensor of n_frames frames and room for s_max labels (the counterpart of ts_ctc_launch_config).
 *   states_per_thread  1 up to 1 024 states (2 s_max + 1), 2 up to 2 048, 4 beyond: ts_ctc_loss's thresholds
 *   threads            round_up(ceil(states / states_per_thread), 64): the workgroup
 *   bp_in_lds          1: the back-pointers (2 bits per frame and state, 16 bytes per frame and wave-slot) live in LDS next to the two state rows;
 *                      0: they do not fit into 160 KiB and go to the workspace
 *   lds_bytes          dynamic LDS of the launch: 4 (2 (states + 4) + states) + 64, plus 16 n_frames states_per_thread threads / 64 when bp_in_lds
 * TS_EINVAL: a NULL pointer, n_frames <= 0, s_max < 0.  TS_EUNSUPPORTED: s_max > 2047. */
int ts_ctc_align_launch_config(int32_t n_frames, int32_t s_max, int32_t* states_per_thread, int32_t* threads, int32_t* bp_in_lds,
                               int32_t* lds_bytes);

/* Bytes of workspace ts_ctc_align needs for this shape (the path's states and log-probabilities, 8 n_frames per utterance, and the back-pointers
 * where they do not fit into LDS), or TS_EINVAL (< 0) for batch <= 0, n_frames <= 0 or s_max < 0, TS_EUNSUPPORTED for s_max > 2047. */
int64_t ts_ctc_align_workspace_bytes(int32_t batch, int32_t n_frames, int32_t s_max);

/* Viterbi forced alignment, one workgroup per utterance.  T = clamp(input_len[b], 0, n_frames), S = clamp(target_len[b], 0, s_max); the states are
 * the blank-extended target (blank, y_0, blank, y_1, ..., blank: 2 S + 1 of them); the path starts in state 0 or 1, ends in one of the last two
 * and maximises the sum of log_softmax(logits[b][:, t])[token of the state at t] over t < T.  State s at frame t is entered from s (stay), from
 * s - 1, and from s - 2 when s is a label state whose label differs from that of s - 2.
 * Ties: stay beats s - 1, s - 1 beats s - 2; the path ends in the last label state unless the final blank state is STRICTLY better; with S = 0
 * the only state is the blank.  (The recursion runs on the raw logits in f32: every path visits every frame once, so the per-frame normaliser
 * shifts all paths alike.  Decisions whose candidates differ by less than the f32 rounding of the partial sums may fall either way.)
 *   path       int32 [B][n_frames]    token id (label or blank) of frame t for t < T; -1 for t >= T, and -1 everywhere for an infeasible utterance
 *   spans      int32 [B][s_max][2]    for target position j < S: first frame and end frame (exclusive) of state 2 j + 1; (0, 0) for j >= S and
 *                                     for infeasible utterances
 *   span_logp  f32 [B][s_max]         sum over the span's frames of log_softmax(logits)[token]; 0 where the span is empty
 *   score      f32 [B]                sum of the path's log-probabilities (0 for T = 0 with S = 0); -inf if infeasible: T < S + the number of
 *                                     equal neighbours in the target, or T = 0 with S > 0
 * Each frame's log-probability is formed in f64 and rounded to f32 once; the sums are f32.  No atomics: equal arguments give equal bits.
 * Logits at t >= T are not read.  targets [B][s_max] holds ids in [0, n_classes) (ts_ctc_prepare's output); an id outside is read as the
 * nearest valid one.  workspace: ts_ctc_align_workspace_bytes bytes, 16-byte aligned; contents are scratch.
 * TS_EINVAL: a NULL pointer (the stream excepted), batch <= 0, n_classes <= 0, n_frames <= 0, s_max < 0, pitch < n_frames, blank outside
 * [0, n_classes).  TS_EUNSUPPORTED: s_max > 2047; workspace not 16-byte aligned. */
int ts_ctc_align(const float* logits, int32_t batch, int32_t n_classes, int32_t n_frames, int32_t pitch, const int32_t* targets, int32_t s_max,
                 const int32_t* input_len, const int32_t* target_len, int32_t blank, int32_t* path, int32_t* spans, float* span_logp, float* score,
                 void* workspace, void* stream);

/* Bytes of workspace ts_ctc_greedy_spans needs (8 n_frames per utterance), or TS_EINVAL (< 0) for batch <= 0 or n_frames <= 0. */
int64_t ts_ctc_greedy_spans_workspace_bytes(int32_t batch, int32_t n_frames);

/* The frame spans of the greedy transcript, one workgroup per utterance, parallel over the frames: argmax over the classes per frame (the lowest
 * index wins ties, as in ts_greedy_decode), runs of equal ids over the frames [0, T), runs of `blank` dropped.  input_len may be NULL: T = n_frames
 * for every utterance (what predict() decodes); otherwise T = clamp(input_len[b], 0, n_frames).
 *   tokens     int32 [B][n_frames]     id of the r-th kept run
 *   spans      int32 [B][n_frames][2]  its first frame and end frame (exclusive)
 *   span_logp  f32 [B][n_frames]       sum over its frames of log_softmax(logits)[id] (each frame formed in f64, rounded once, summed in f32 in
 *                                      frame order)
 *   counts     int32 [B]               number of kept runs
 * Entries at or beyond counts[b] are zero.  workspace: ts_ctc_greedy_spans_workspace_bytes bytes, 4-byte aligned; contents are scratch.
 * TS_EINVAL: a NULL pointer (input_len and the stream excepted), batch <= 0, n_classes <= 0, n_frames <= 0, pitch < n_frames, blank outside
 * [0, n_classes).  TS_EUNSUPPORTED: workspace not 4-byte aligned. */
int ts_ctc_greedy_spans(const float* logits, int32_t batch, int32_t n_classes, int32_t n_frames, int32_t pitch, const int32_t* input_len,
                        int32_t blank, int32_t* tokens, int32_t* spans, float* span_logp, int32_t* counts, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* THUNDER_SPEECH_AMD_CTC_ALIGN_H */
