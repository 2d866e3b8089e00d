"""CTC prefix beam search with n-best output on the GPU (no reference counterpart; the reference's `predict` decodes greedily,
src/thunder/module.py:98-101).

`beam_search` runs the three launches of csrc/ctc_beam.hip (frame candidates, the search with one workgroup per utterance, the
backtrace) on the logits `calculate_ctc` takes ([B, V, T'] BEFORE softmax) and returns a dataclass of DEVICE tensors; the host side
(`BeamToken`, `Hypothesis`, `hypotheses_from_tables`) is what `BaseCTCModule.predict_nbest` hands to users.  The algorithm is
specified in thunder_speech_amd/ctc_beam.h.  There is no CPU path."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, List, Optional

import torch
from torch import Tensor

from . import _lib
from .ctc_align import _logits_f32


@dataclass
class BeamResult:
    """Device tensors of `beam_search` (thunder_speech_amd/ctc_beam.h: ts_ctc_beam_search); entries beyond a length or a count are zero, scores beyond
    the count are -inf."""
    tokens: Tensor        # int32 [B, n_best, T']   class ids, forward order
    frames: Tensor        # int32 [B, n_best, T']   frame at which each token entered its hypothesis
    lengths: Tensor       # int32 [B, n_best]
    scores: Tensor        # f32 [B, n_best]         log of the summed probability of the hypothesis's alignments
    counts: Tensor        # int32 [B]               hypotheses produced, best first


@dataclass
class BeamToken:
    token: str
    frame: int
    time: float           # seconds: frame * samples_per_frame / sample_rate


@dataclass
class Hypothesis:
    text: str
    score: float
    tokens: List[BeamToken] = field(default_factory=list)
    lm_score: Optional[float] = None      # unweighted log10 LM score (tokens and </s>) of a search with LM fusion (ctc_lm.py); None without


def beam_search(logits: Tensor, lengths: Optional[Tensor] = None, blank_idx: int = 0, beam_width: int = 16, token_cap: int = 8,
                n_best: int = 1) -> BeamResult:
    """The `n_best` most probable transcripts of each clip under CTC prefix beam search with `beam_width` prefixes and, per frame, the
    blank and the `token_cap` most probable other classes.  `lengths` None: every frame (as `predict` decodes)."""
    lg = _logits_f32(logits, "beam_search")
    b, v, t = lg.shape
    if b == 0 or t == 0:
        raise ValueError("beam_search: empty logits")
    dev = lg.device
    il = None if lengths is None else lengths.to(device=dev, dtype=torch.int64).to(torch.int32).contiguous()
    L = _lib.lib()
    nbytes = L.ts_ctc_beam_workspace_bytes(b, t, int(beam_width), int(token_cap))
    if nbytes < 0:
        _lib.check(int(nbytes), "ts_ctc_beam_workspace_bytes")
    n_best = int(n_best)
    if not 1 <= n_best <= int(beam_width):
        raise ValueError("beam_search: 1 <= n_best <= beam_width required")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    tokens = torch.empty(b, n_best, t, dtype=torch.int32, device=dev)
    frames = torch.empty(b, n_best, t, dtype=torch.int32, device=dev)
    out_len = torch.empty(b, n_best, dtype=torch.int32, device=dev)
    scores = torch.empty(b, n_best, dtype=torch.float32, device=dev)
    counts = torch.empty(b, dtype=torch.int32, device=dev)
    st = L.ts_ctc_beam_search(lg.data_ptr(), b, v, t, lg.stride(1), None if il is None else il.data_ptr(), int(blank_idx), int(beam_width),
                              int(token_cap), n_best, tokens.data_ptr(), frames.data_ptr(), out_len.data_ptr(), scores.data_ptr(),
                              counts.data_ptr(), ws.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(st, "ts_ctc_beam_search")
    return BeamResult(tokens, frames, out_len, scores, counts)


def hypotheses_from_tables(tokens, frames, lengths, scores, counts, itos: List[str], to_text: Callable[[List[int]], str], samples_per_frame: int,
                           sample_rate: int, lm_scores=None) -> List[List[Hypothesis]]:
    """Host tables (numpy: tokens / frames [B, N, T'], lengths / scores [B, N], counts [B]) -> per clip its hypotheses, best first.
    `to_text` joins ids into the transcript (the text transform's rule); frame f is at f * samples_per_frame / sample_rate seconds.
    `lm_scores` [B, N], of a search with LM fusion, fills `lm_score`."""
    out = []
    for b in range(len(counts)):
        clip = []
        for n in range(int(counts[b])):
            ln = int(lengths[b, n])
            ids = [int(i) for i in tokens[b, n, :ln]]
            toks = [BeamToken(itos[i], int(f), int(f) * samples_per_frame / sample_rate) for i, f in zip(ids, frames[b, n, :ln])]
            clip.append(Hypothesis(to_text(ids), float(scores[b, n]), toks, None if lm_scores is None else float(lm_scores[b, n])))
        out.append(clip)
    return out
