"""CTC forced alignment and greedy token spans on the GPU: "when was it said" (no reference counterpart; the reference's
`predict` returns bare strings, src/thunder/module.py:98-101).

`forced_align` runs the Viterbi recursion of csrc/ctc_align.hip over the blank-extended target (one workgroup per utterance,
back-pointers in LDS, the backtrace on the device) and `greedy_spans` keeps the frame positions `ts_greedy_decode` throws away.
Both take the logits `calculate_ctc` takes ([B, V, T'] BEFORE softmax) and return small dataclasses of DEVICE tensors; the host
side (`TokenSpan`, `AlignedClip`, `words`) is what `BaseCTCModule.align` / `predict_spans` hand to users.  There is no CPU path."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

import torch
from torch import Tensor

from . import _lib
from .ctc_loss import _prepare_on_device, _prepare_targets

WORD_SEPARATORS = (" ", "|", "▁")       # what BatchTextTransformer.decode_prediction turns into spaces


@dataclass
class Alignment:
    """Device tensors of `forced_align` (thunder_speech_amd/ctc_align.h: ts_ctc_align)."""
    path: Tensor          # int32 [B, T']     token id per frame, -1 beyond the clip's length and for infeasible clips
    spans: Tensor         # int32 [B, S, 2]   first and end frame (exclusive) of each target position, (0, 0) beyond the target's length
    span_logp: Tensor     # f32 [B, S]        sum of the span's log-probabilities
    score: Tensor         # f32 [B]           sum of the path's log-probabilities, -inf for an infeasible clip
    targets: Tensor       # int32 [B, S]      the label ids the kernel read (after ts_ctc_prepare's rules)
    target_lengths: Tensor    # int32 [B]     their lengths, clamped to [0, S]


@dataclass
class GreedySpans:
    """Device tensors of `greedy_spans` (thunder_speech_amd/ctc_align.h: ts_ctc_greedy_spans); entries at or beyond counts[b] are zero."""
    tokens: Tensor        # int32 [B, T']
    spans: Tensor         # int32 [B, T', 2]
    span_logp: Tensor     # f32 [B, T']
    counts: Tensor        # int32 [B]


@dataclass
class TokenSpan:
    token: str
    start: float          # seconds
    end: float            # seconds (exclusive)
    start_frame: int
    end_frame: int        # exclusive
    logp: float


@dataclass
class AlignedClip:
    score: float
    tokens: List[TokenSpan] = field(default_factory=list)


def _logits_f32(logits: Tensor, what: str) -> Tensor:
    if not logits.is_cuda:
        raise RuntimeError(f"{what}: GPU tensors required (no CPU fallback)")
    if logits.dim() != 3:
        raise ValueError(f"{what}: logits must be [batch, vocab, time]")
    lg = logits.detach()
    if lg.dtype != torch.float32 or lg.stride(2) != 1 or lg.stride(0) != lg.shape[1] * lg.stride(1):
        lg = lg.to(torch.float32).contiguous()
    return lg


def forced_align(logits: Tensor, targets: Tensor, input_lengths: Tensor, target_lengths: Tensor, blank_idx: int) -> Alignment:
    """Best CTC path of each transcript through its clip.  Arguments as `calculate_ctc`: logits [B, V, T'] before softmax, targets
    [B, S] padded or the 1-D concatenation, lengths of any integer or float dtype; targets and lengths go through the loss's own
    preparation (a device transcript with an id outside [0, V) becomes infeasible: score -inf, no spans)."""
    return _forced_align("forced_align", logits, targets, input_lengths, target_lengths, blank_idx, None)


def forced_align_long(logits: Tensor, targets: Tensor, input_lengths: Tensor, target_lengths: Tensor, blank_idx: int,
                      states_per_thread: int = 0) -> Alignment:
    """`forced_align` on ts_ctc_align_long (thunder_speech_amd/longform.h): the same arguments, results, tie rules and arithmetic, for
    transcripts of up to 32 767 labels where `forced_align` refuses more than 2 047.  `states_per_thread` 0: chosen from the label
    capacity; 8, 16, 32 or 64: that instantiation."""
    return _forced_align("forced_align_long", logits, targets, input_lengths, target_lengths, blank_idx, int(states_per_thread))


def _forced_align(what: str, logits: Tensor, targets: Tensor, input_lengths: Tensor, target_lengths: Tensor, blank_idx: int,
                  states_per_thread: Optional[int]) -> Alignment:
    """The two aligners' shared preparation and call; states_per_thread None: ts_ctc_align, else ts_ctc_align_long."""
    lg = _logits_f32(logits, what)
    b, v, t = lg.shape
    if b == 0 or t == 0:
        raise ValueError(f"{what}: empty logits")
    dev = lg.device
    if targets.is_cuda and targets.dim() == 2:
        tg, tl, il = _prepare_on_device(targets, target_lengths, input_lengths, b, v, dev)
    else:
        tg, tl, bad_rows = _prepare_targets(targets, target_lengths, b, v, dev)
        il = input_lengths.to(device=dev, dtype=torch.int64).to(torch.int32).contiguous()
        if bad_rows is not None:
            il = torch.where(bad_rows, torch.zeros_like(il), il)
            tl = torch.where(bad_rows & (tl == 0), torch.ones_like(tl), tl)
    s_max = tg.shape[1]
    L = _lib.lib()
    name = "ts_ctc_align" if states_per_thread is None else "ts_ctc_align_long"
    nbytes = getattr(L, name + "_workspace_bytes")(b, t, s_max)
    if nbytes < 0:
        _lib.check(int(nbytes), name + "_workspace_bytes")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    path = torch.empty(b, t, dtype=torch.int32, device=dev)
    spans = torch.empty(b, s_max, 2, dtype=torch.int32, device=dev)
    span_logp = torch.empty(b, s_max, dtype=torch.float32, device=dev)
    score = torch.empty(b, dtype=torch.float32, device=dev)
    head = (lg.data_ptr(), b, v, t, lg.stride(1), tg.data_ptr(), s_max, il.data_ptr(), tl.data_ptr(), int(blank_idx))
    tail = (path.data_ptr(), spans.data_ptr(), span_logp.data_ptr(), score.data_ptr(), ws.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    st = L.ts_ctc_align(*head, *tail) if states_per_thread is None else L.ts_ctc_align_long(*head, states_per_thread, *tail)
    _lib.check(st, name)
    return Alignment(path, spans, span_logp, score, tg, tl.clamp(0, s_max))


def greedy_spans(logits: Tensor, lengths: Optional[Tensor] = None, blank_idx: int = 0) -> GreedySpans:
    """The greedy transcript with its frame spans: argmax per frame, runs of equal ids over the first `lengths[b]` frames (None: every
    frame, as `predict` decodes), blank runs dropped."""
    lg = _logits_f32(logits, "greedy_spans")
    b, v, t = lg.shape
    if b == 0 or t == 0:
        raise ValueError("greedy_spans: empty logits")
    dev = lg.device
    il = None if lengths is None else lengths.to(device=dev, dtype=torch.int64).to(torch.int32).contiguous()
    L = _lib.lib()
    ws = torch.empty(L.ts_ctc_greedy_spans_workspace_bytes(b, t), dtype=torch.uint8, device=dev)
    tokens = torch.empty(b, t, dtype=torch.int32, device=dev)
    spans = torch.empty(b, t, 2, dtype=torch.int32, device=dev)
    span_logp = torch.empty(b, t, dtype=torch.float32, device=dev)
    counts = torch.empty(b, dtype=torch.int32, device=dev)
    st = L.ts_ctc_greedy_spans(lg.data_ptr(), b, v, t, lg.stride(1), None if il is None else il.data_ptr(), int(blank_idx), tokens.data_ptr(),
                               spans.data_ptr(), span_logp.data_ptr(), counts.data_ptr(), ws.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(st, "ts_ctc_greedy_spans")
    return GreedySpans(tokens, spans, span_logp, counts)


def _to_host(*tensors: Tensor):
    """The tensors on the host after ONE device -> host copy: all are 4-byte types, so they travel as one int32 buffer."""
    flat = torch.cat([t.contiguous().view(torch.int32).reshape(-1) for t in tensors]).cpu()
    out, at = [], 0
    for t in tensors:
        n = t.numel()
        out.append(flat[at: at + n].view(t.dtype).reshape(t.shape).numpy())
        at += n
    return out


def clips_from_spans(ids, spans, logp, counts, scores, itos: List[str], samples_per_frame: int, sample_rate: int) -> List[AlignedClip]:
    """Host tables (numpy: ids [B, N], spans [B, N, 2], logp [B, N], counts [B], scores [B]) -> one AlignedClip per row; frame f is at
    f * samples_per_frame / sample_rate seconds."""
    clips = []
    for b in range(len(counts)):
        clip = AlignedClip(score=float(scores[b]))
        for j in range(int(counts[b])):
            f0, f1 = int(spans[b, j, 0]), int(spans[b, j, 1])
            clip.tokens.append(TokenSpan(itos[int(ids[b, j])], f0 * samples_per_frame / sample_rate, f1 * samples_per_frame / sample_rate, f0, f1,
                                         float(logp[b, j])))
        clips.append(clip)
    return clips


def words(clip: AlignedClip) -> List[TokenSpan]:
    """Token spans merged into words at the separators `decode_prediction` turns into spaces (" ", "|", "▁"): a separator token ends
    the word before it, a sentencepiece token that begins with "▁" starts a new one.  A word runs from its first token's start to
    its last token's end; its logp is the sum."""
    out: List[TokenSpan] = []
    cur: Optional[TokenSpan] = None
    for tok in clip.tokens:
        text = tok.token
        if text in WORD_SEPARATORS:
            cur = None
            continue
        if text.startswith("▁"):
            cur, text = None, text[1:]
        if cur is None:
            cur = TokenSpan(text, tok.start, tok.end, tok.start_frame, tok.end_frame, tok.logp)
            out.append(cur)
        else:
            cur.token += text
            cur.end, cur.end_frame, cur.logp = tok.end, tok.end_frame, cur.logp + tok.logp
    return out
