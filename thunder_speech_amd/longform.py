"""Recordings longer than one forward pass (no reference counterpart; the reference's `predict` takes one batch of clips that fit one
pass, src/thunder/module.py:88-100): the window plan (host arithmetic) and the two plumbing launches of csrc/longform.hip around the
forward (include_open/thunder_speech_amd/longform.h).  `BaseCTCModule.logits_long` / `transcribe_long` / `predict_spans_long` /
`align_long` are built on these; the long aligner is `ctc_align.forced_align_long`.

A recording is run as overlapping windows of ONE length (`chunk_samples`), every one starting on the recording's frame grid (a multiple
of `samples_per_frame`), so that local frame j of a window starting at sample s is global frame s / samples_per_frame + j: the frame
grid of the recording run whole.  The last window is moved back so that it ends at the recording's end: no window is padded by more
than a frame's worth of zeros, no family sees a short clip, and one [batch, chunk] signature -- one captured inference graph -- serves
every batch.  Neighbours are cut in the middle of their overlap; every global frame comes from exactly one window.

Out of scope: choosing the seams from the data (cutting where both windows are most blank), streaming input that never resides on the
device as a whole, transcripts beyond the aligner's cap (thunder_speech_amd/longform.h: TS_CTC_ALIGN_LONG_S_MAX labels)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence

import torch
from torch import Tensor

from . import _lib


@dataclass
class WindowPlan:
    """Where the windows of one recording sit (host integers).  Window w starts at sample starts[w] = frames[w] * samples_per_frame and
    owns the global frames [cut_lo[w], cut_hi[w]); cut_lo[0] = 0 and cut_hi[-1] = n_frames, the stitched length T_r."""
    n_samples: int
    chunk_samples: int
    samples_per_frame: int
    frames_per_window: int
    hop_frames: int
    starts: List[int]
    frames: List[int]
    cut_lo: List[int]
    cut_hi: List[int]

    @property
    def n_frames(self) -> int:
        return self.cut_hi[-1]

    def __len__(self) -> int:
        return len(self.starts)


def plan_windows(n_samples: int, chunk_samples: int, context_frames: int, samples_per_frame: int, frames_per_window: int,
                 grid_multiple: int = 1) -> Optional[WindowPlan]:
    """The windows of a recording of `n_samples` samples, or None for one that fits a single window (n_samples <= chunk_samples: it is run
    as one clip of its own length).  `frames_per_window` (F) is the number of output frames of a window of `chunk_samples`, by the module's
    own length arithmetic.  hop_frames = F - 2 context_frames; regular windows sit at global frames w * hop_frames below g_last, the last one
    at g_last = ceil((n_samples - chunk_samples) / samples_per_frame); the seam between neighbours is (g_w + F + g_{w+1}) // 2.
    `grid_multiple` m > 1: the family's frame grid closes only at multiples of m frames (SEW's squeeze_factor, an adapter's total stride):
    hop_frames must be a multiple of m, and g_last is rounded up to one.  ValueError for a plan that cannot be made."""
    n, chunk, ctx, spf, f, m = (int(v) for v in (n_samples, chunk_samples, context_frames, samples_per_frame, frames_per_window, grid_multiple))
    if chunk <= 0 or spf <= 0 or f <= 0 or ctx < 0 or m <= 0 or n < 0:
        raise ValueError(f"plan_windows: chunk_samples {chunk}, samples_per_frame {spf}, frames_per_window {f} and grid_multiple {m} must be "
                         f"positive, context_frames {ctx} and n_samples {n} not negative")
    hop = f - 2 * ctx
    if hop < 1:
        raise ValueError(f"plan_windows: a window of {f} frames leaves no hop under a context of {ctx} frames on either side "
                         f"(hop_frames = {hop}); use a longer chunk or a shorter context")
    if hop % m:
        raise ValueError(f"plan_windows: hop_frames = {hop} is not a multiple of {m}, the step of this family's frame grid (SEW: "
                         f"squeeze_factor; add_adapter: adapter_stride ** num_adapter_layers); change the chunk or the context")
    if n <= chunk:
        return None
    g_last = -(-(n - chunk) // (spf * m)) * m
    frames = list(range(0, g_last, hop)) + [g_last]
    cuts = [(frames[w] + f + frames[w + 1]) // 2 for w in range(len(frames) - 1)]
    return WindowPlan(n, chunk, spf, f, hop, [g * spf for g in frames], frames, [0] + cuts, cuts + [g_last + f])


def grid_multiple(config) -> int:
    """The step of a transformers family's frame grid in output frames, from its config (None, or a mel family's: 1): SEW pools
    `squeeze_factor` frames in front of its encoder, an adapter strides by adapter_stride ** num_adapter_layers."""
    m = 1
    if config is None:
        return m
    if int(getattr(config, "squeeze_factor", 1) or 1) > 1:
        m *= int(config.squeeze_factor)
    if getattr(config, "add_adapter", False):
        m *= int(config.adapter_stride) ** int(config.num_adapter_layers)
    return m


def pack_recordings(recordings: Sequence[Tensor]):
    """(audio f32 [sum n_r], rec_begin int64 [R + 1] on the device, the lengths on the host) of 1-D GPU waveforms: ts_longform_gather's input."""
    lengths = [int(r.shape[0]) for r in recordings]
    audio = recordings[0].contiguous() if len(recordings) == 1 else torch.cat(list(recordings))
    begin = [0]
    for n in lengths:
        begin.append(begin[-1] + n)
    return audio, torch.tensor(begin, dtype=torch.int64).to(audio.device, non_blocking=True), lengths


def gather_windows(audio: Tensor, rec_begin: Tensor, windows: Tensor, n_windows: int, out: Tensor) -> None:
    """ts_longform_gather: rows [0, n_windows) of `out` [batch, chunk] from `windows` int64 [>= n_windows, 2] (recording, start sample); the
    other rows and every sample past a recording's end are zeros.  `out` is written in place: it is the staging buffer the graphs are keyed by."""
    if not (audio.is_cuda and out.is_cuda and rec_begin.is_cuda and windows.is_cuda):
        raise RuntimeError("gather_windows: GPU tensors required (no CPU fallback)")
    if audio.dtype != torch.float32 or out.dtype != torch.float32 or not out.is_contiguous() or not audio.is_contiguous():
        raise ValueError("gather_windows: audio and out must be contiguous float32")
    if rec_begin.dtype != torch.int64 or windows.dtype != torch.int64 or not windows.is_contiguous() or n_windows > windows.shape[0]:
        raise ValueError("gather_windows: rec_begin and windows must be int64, windows [>= n_windows, 2] contiguous")
    st = _lib.lib().ts_longform_gather(audio.data_ptr(), rec_begin.data_ptr(), rec_begin.numel() - 1, windows.data_ptr(), int(n_windows),
                                       out.data_ptr(), out.shape[0], out.shape[1], torch.cuda.current_stream(out.device).cuda_stream)
    _lib.check(st, "ts_longform_gather")


def cut_table(plans: Sequence[Optional[WindowPlan]]) -> List[List[int]]:
    """ts_longform_stitch's table, rows (recording, g_w, cut_lo, cut_hi) in window order, for the recordings that have a plan."""
    return [[r, p.frames[w], p.cut_lo[w], p.cut_hi[w]] for r, p in enumerate(plans) if p is not None for w in range(len(p))]


def stitch_windows(win_logits: Tensor, cuts: Tensor, out: Tensor, lengths: Tensor) -> None:
    """ts_longform_stitch: `win_logits` [W, V, F] (bf16 or f32) -> `out` f32 [R, V, pitch] and `lengths` int32 [R] by `cuts` int32 [W, 4];
    rows of recordings without a window are left as they are."""
    if not (win_logits.is_cuda and cuts.is_cuda and out.is_cuda and lengths.is_cuda):
        raise RuntimeError("stitch_windows: GPU tensors required (no CPU fallback)")
    if win_logits.dtype not in (torch.float32, torch.bfloat16) or not win_logits.is_contiguous() or win_logits.dim() != 3:
        raise ValueError("stitch_windows: window logits must be contiguous [W, V, F], float32 or bfloat16")
    if out.dtype != torch.float32 or not out.is_contiguous() or out.dim() != 3 or out.shape[1] != win_logits.shape[1]:
        raise ValueError("stitch_windows: out must be contiguous float32 [R, V, pitch]")
    if cuts.dtype != torch.int32 or not cuts.is_contiguous() or tuple(cuts.shape) != (win_logits.shape[0], 4):
        raise ValueError("stitch_windows: cuts must be contiguous int32 [W, 4]")
    if lengths.dtype != torch.int32 or not lengths.is_contiguous() or lengths.numel() != out.shape[0]:
        raise ValueError("stitch_windows: lengths must be contiguous int32 [R]")
    w, v, f = win_logits.shape
    st = _lib.lib().ts_longform_stitch(win_logits.data_ptr(), int(win_logits.dtype == torch.bfloat16), w, v, f, cuts.data_ptr(), out.data_ptr(),
                                       out.shape[0], out.shape[2], lengths.data_ptr(), torch.cuda.current_stream(out.device).cuda_stream)
    _lib.check(st, "ts_longform_stitch")


@dataclass
class LongLogits:
    """What `BaseCTCModule.logits_long` returns: the stitched logits on each recording's own frame grid."""
    logits: Tensor                          # f32 [R, V, T_max], zeros beyond a recording's length
    lengths: Tensor                         # int32 [R]
    plans: List[Optional[WindowPlan]]       # None for a recording that fits one window (it ran as one clip of its own length)
