/*
 * thunder_speech_amd/longform.h -- companion C ABI of include/thunder_speech_amd.h: recordings longer than one forward pass.  Two plumbing
 * launches that take a recording through the model as overlapping, full-length windows (ts_longform_gather in front of the forward,
 * ts_longform_stitch behind it) and a Viterbi aligner whose label capacity is not bounded by four states per thread (ts_ctc_align_long), in
 * csrc/longform.hip and csrc/ctc_align_long.hip.  The same shared library exports these entry points; the conventions are the core header's
 * (DEVICE pointers into caller-owned buffers, `stream` a hipStream_t passed as void*, 0 / TS_EINVAL / TS_EUNSUPPORTED / positive hipError_t
 * returns, nothing allocates, frees or synchronises, so every call can be captured into a hipGraph).  The core ABI (TS_ABI_VERSION) and the
 * other companions, ctc_align.h included, are unchanged by this header; it is versioned on its own by TS_LONGFORM_ABI_VERSION.
 *
 * No reference call site: the reference's predict takes one batch of clips that fit one forward pass (module.py:88-100).  The window plan itself
 * (where the windows start, where neighbours are cut) is host arithmetic and lives with the caller (thunder_speech_amd/longform.py); the two
 * plumbing launches take it as tables.
 * Out of scope: choosing the seams from the data, streaming input that never resides on the device as a whole, transcripts beyond the
 * aligner's cap of TS_CTC_ALIGN_LONG_S_MAX labels.
 */
#ifndef THUNDER_SPEECH_AMD_LONGFORM_H
#define THUNDER_SPEECH_AMD_LONGFORM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TS_LONGFORM_ABI_VERSION 1

/* Label capacity of ts_ctc_align_long: 2 * 32 767 + 1 = 65 535 states, 64 per thread of a 1 024-thread workgroup (the instantiation with 64
 * states per thread needs no scratch memory: 127 of the 128 VGPRs a wave of that workgroup may hold, as -Rpass-analysis=kernel-resource-usage
 * reports them). */
#define TS_CTC_ALIGN_LONG_S_MAX 32767
/* Class capacity of ts_ctc_align_long: 16 staged frames x n_classes f32 logits must fit into the 160 KiB of LDS next to the boundary cells. */
#define TS_CTC_ALIGN_LONG_V_MAX 2400

/* Version of this companion ABI (a binder checks it next to ts_abi_version). */
int ts_longform_abi_version(void);

/* Copy full-length windows out of packed audio into one staging buffer, one launch.
 *   audio        f32, the samples of n_recordings recordings back to back (any alignment of the pieces)
 *   rec_begin    int64 [n_recordings + 1]: recording r is audio[rec_begin[r] .. rec_begin[r + 1])
 *   windows      int64 [n_windows][2]: (recording, start sample within it) of the window that becomes row i of `out`
 *   out          f32 [batch][chunk]: row i < n_windows holds the recording's samples start .. start + chunk, samples at or past the recording's
 *                end (and before its begin, for a negative start) as zeros; rows n_windows .. batch are zeros; a row whose recording index is
 *                outside [0, n_recordings) is zeros.  16-byte stores where `out` and chunk allow, 16-byte loads where the source piece does.
 * Nothing outside out[batch][chunk] is written.
 * TS_EINVAL: a NULL pointer (the stream excepted), n_recordings <= 0, n_windows < 0, batch <= 0, n_windows > batch, chunk <= 0.
 * TS_EUNSUPPORTED: audio or out not 4-byte aligned, rec_begin or windows not 8-byte aligned, batch > 65535 (the launch's grid). */
int ts_longform_gather(const float* audio, const int64_t* rec_begin, int32_t n_recordings, const int64_t* windows, int32_t n_windows, float* out,
                       int32_t batch, int32_t chunk, void* stream);

/* Assemble the windows' logits into one logit sequence per recording on the recording's frame grid, one launch, no atomics.
 *   win          [n_windows][n_classes][frames_per_window], bf16 when in_bf16 != 0, else f32: what the forward returned for the windows
 *   cuts         int32 [n_windows][4]: per window (recording r, g_w, cut_lo, cut_hi): window w starts at global frame g_w of recording r and
 *                owns the global frames [cut_lo, cut_hi).  The windows of a recording are consecutive rows in time order; the caller's plan
 *                makes the ranges of a recording disjoint, gap-free from 0 and inside their windows.  Read defensively: a range is clipped to
 *                [max(g_w, 0), min(g_w + frames_per_window, pitch)), a row whose recording is outside [0, n_recordings) is skipped.
 *   out          f32 [n_recordings][n_classes][pitch]: out[r][v][g] = win[w][v][g - g_w] for g in window w's range; the recording's last window
 *                (the last row that names r) also writes 0 to [its cut_hi, pitch).  Rows of recordings that no window names are not written.
 *   lengths      int32 [n_recordings]: the last window's cut_hi (clipped as above), the stitched length T_r; not written for a recording
 *                without a window
 * Accesses are coalesced along time.
 * TS_EINVAL: a NULL pointer (the stream excepted), n_windows <= 0, n_classes <= 0, frames_per_window <= 0, n_recordings <= 0, pitch <= 0,
 * n_classes > 65535 (the launch's grid).  TS_EUNSUPPORTED: win not aligned to its element, cuts / out / lengths not 4-byte aligned. */
int ts_longform_stitch(const void* win, int32_t in_bf16, int32_t n_windows, int32_t n_classes, int32_t frames_per_window, const int32_t* cuts,
                       float* out, int32_t n_recordings, int32_t pitch, int32_t* lengths, void* stream);

/* Host only: what ts_ctc_align_long launches.
 *   states_per_thread_in  0: chosen from s_max, the smallest of 8, 16, 32, 64 under which the 2 s_max + 1 states fit 1 024 threads (8 up to
 *                         8 192 states, 16 up to 16 384, 32 up to 32 768, 64 beyond); or one of 8, 16, 32, 64, taken as given
 *   states_per_thread     the value in use
 *   threads               round_up(ceil(states / states_per_thread), 64): the workgroup
 *   lds_bytes             dynamic LDS of the launch: 64 n_classes (the staged logits: 16 frames x n_classes f32) + 8 (threads + 1) (the boundary
 *                         cells, double-buffered) + 64 + 16
 * TS_EINVAL: a NULL pointer, n_frames <= 0, s_max < 0, n_classes <= 0, states_per_thread_in not one of 0, 8, 16, 32, 64, or given and too small
 * (2 s_max + 1 > 1 024 states_per_thread_in).  TS_EUNSUPPORTED: s_max > TS_CTC_ALIGN_LONG_S_MAX, n_classes > TS_CTC_ALIGN_LONG_V_MAX.  The
 * refusals are made in this order: NULL and ranges, then the caps, then states_per_thread_in against s_max. */
int ts_ctc_align_long_launch_config(int32_t n_frames, int32_t s_max, int32_t states_per_thread_in, int32_t n_classes, int32_t* states_per_thread,
                                    int32_t* threads, int32_t* lds_bytes);

/* Bytes of workspace ts_ctc_align_long needs for this shape, whatever states_per_thread: per utterance and frame the back-pointers, 2 bits per
 * state in rows of round_up(2 s_max + 1, 64) / 4 bytes, and the path's state and log-probability (8 bytes).  TS_EINVAL (< 0) for batch <= 0,
 * n_frames <= 0 or s_max < 0, TS_EUNSUPPORTED for s_max > TS_CTC_ALIGN_LONG_S_MAX. */
int64_t ts_ctc_align_long_workspace_bytes(int32_t batch, int32_t n_frames, int32_t s_max);

/* ts_ctc_align (thunder_speech_amd/ctc_align.h) for transcripts of up to TS_CTC_ALIGN_LONG_S_MAX labels: the same inputs, the same outputs
 * (path, spans, span_logp, score, -inf and -1 / (0, 0) / 0 for an infeasible utterance), the same tie rules (stay beats s - 1, s - 1 beats s - 2,
 * the path ends in the last label state unless the final blank state is STRICTLY better) and the same arithmetic (the recursion on the raw f32
 * logits, each path frame's log-probability formed in f64 and rounded to f32 once, f32 sums, no atomics) -- see that header for every
 * argument; on a shape both accept, path and spans are equal and the sums differ by their order only.
 * Only the layout differs.  One workgroup of up to 1 024 threads per utterance and no waiting across workgroups; each thread owns
 * states_per_thread CONTIGUOUS states in registers and updates them in place from the high state down, so per frame one value per thread (its
 * highest state; the block starts on a blank state, which is never skipped into) crosses to its neighbour through LDS, behind one LDS-ordering
 * barrier.  A frame's n_classes logits are staged in LDS once, requested 8 frames ahead of their use, and the states read their token's cell there.
 * The back-pointers go to the workspace, one store of 2 states_per_thread bits per thread and frame; the backtrace fetches 16 frames per
 * round trip.
 *   states_per_thread   0 (chosen from s_max) or 8, 16, 32, 64: ts_ctc_align_long_launch_config's states_per_thread_in
 *   workspace           ts_ctc_align_long_workspace_bytes bytes, 16-byte aligned; contents are scratch
 * TS_EINVAL: a NULL pointer (the stream excepted), batch <= 0, n_classes <= 0, n_frames <= 0, s_max < 0, pitch < n_frames, blank outside
 * [0, n_classes), states_per_thread not one of 0, 8, 16, 32, 64 or too small for s_max.  TS_EUNSUPPORTED: s_max > TS_CTC_ALIGN_LONG_S_MAX,
 * n_classes > TS_CTC_ALIGN_LONG_V_MAX, workspace not 16-byte aligned.  All of these return before any device call. */
int ts_ctc_align_long(const float* logits, int32_t batch, int32_t n_classes, int32_t n_frames, int32_t pitch, const int32_t* targets,
                      int32_t s_max, const int32_t* input_len, const int32_t* target_len, int32_t blank, int32_t states_per_thread, int32_t* path,
                      int32_t* spans, float* span_logp, float* score, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* THUNDER_SPEECH_AMD_LONGFORM_H */
