"""Token-level n-gram shallow fusion for the CTC beam search (no reference counterpart).

The LM's words are the acoustic model's CTC classes: characters for QuartzNet and wav2vec2, sentencepiece pieces for Citrinet.  The host side
(this module, numpy only) reads an ARPA file (`read_arpa`), matches its words to the classes and compiles the table to a back-off automaton
(`NGramLM`); `NGramLM.weights(alpha, beta)` forms the f64 factors of one setting on the host, so that the device takes no exp and no log of the
LM, and `beam_search_lm` runs the three launches of csrc/ctc_beam_lm.hip on them.  The algorithm is specified in thunder_speech_amd/ctc_beam_lm.h.  There is
no CPU path for the search.

For the character vocabularies (QuartzNet, the wav2vec2 family) the second half of this module fuses a WORD-level ARPA LM instead: `WordNGramLM`
compiles the words to the same automaton (word ids as classes) and spells them into a lexicon trie, with hot words; `beam_search_word_lm` runs
csrc/ctc_beam_word_lm.hip on them (thunder_speech_amd/ctc_beam_word_lm.h).  For the sentencepiece vocabularies (Citrinet, NeMo word-piece checkpoints
after `fix_vocab`) the third part does the same with a trie over LETTERS: `PieceWordNGramLM` reads the same word-level ARPA file, a piece that
begins with U+2581 starts a word, and `beam_search_piece_lm` runs csrc/ctc_beam_piece_lm.hip (thunder_speech_amd/ctc_beam_piece_lm.h); the
token-level `NGramLM` over pieces remains for LMs that were trained on pieces."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Any, Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from .ctc_beam import BeamResult

BOS, EOS, UNK = -1, -2, -3                       # ids of <s>, </s>, <unk> inside n-grams; classes are >= 0
_SPECIAL = {"<s>": BOS, "</s>": EOS, "<unk>": UNK}
NGram = Tuple[int, ...]


def read_arpa(path_or_text: str) -> Tuple[int, List[Dict[Tuple[str, ...], Tuple[float, float]]]]:
    """Standard ARPA text (a path, or the text itself if it holds a line break) -> (order, tables): tables[n - 1] maps every n-gram (a tuple of
    words) to (log10 p, log10 back-off).  A missing back-off reads as 0; the highest order has none.  ValueError, naming the line, on malformed
    input."""
    if "\n" in path_or_text:
        text = path_or_text
    else:
        with open(path_or_text, encoding="utf-8") as f:
            text = f.read()
    counts: Dict[int, int] = {}
    tables: Dict[int, Dict[Tuple[str, ...], Tuple[float, float]]] = {}
    section, seen_data, ended = None, False, False       # section: None before \data\, 0 in the counts, n in \n-grams:
    for no, raw in enumerate(text.splitlines(), 1):
        line = raw.strip()
        if not line:
            continue
        if ended:
            raise ValueError(f"read_arpa: line {no}: text after \\end\\: {line!r}")
        if line == "\\data\\":
            if seen_data:
                raise ValueError(f"read_arpa: line {no}: a second \\data\\")
            seen_data, section = True, 0
            continue
        if not seen_data:
            continue                                     # ARPA allows a preamble before \data\
        if line == "\\end\\":
            ended = True
            continue
        if line.startswith("\\"):
            head = line[1:-1].split("-")[0] if line.endswith("-grams:") else ""
            if not head.isdigit() or int(head) < 1:
                raise ValueError(f"read_arpa: line {no}: unknown section {line!r}")
            n = int(head)
            if n not in counts:
                raise ValueError(f"read_arpa: line {no}: \\{n}-grams: without an `ngram {n}=` count")
            if n in tables or n != len(tables) + 1:
                raise ValueError(f"read_arpa: line {no}: \\{n}-grams: out of order")
            section, tables[n] = n, {}
            continue
        if section == 0:
            body = line.replace(" ", "").replace("\t", "")
            if not body.startswith("ngram") or "=" not in body:
                raise ValueError(f"read_arpa: line {no}: expected `ngram N=count`, got {line!r}")
            n, _, cnt = body[5:].partition("=")
            if not n.isdigit() or not cnt.isdigit() or int(n) < 1 or int(n) in counts:
                raise ValueError(f"read_arpa: line {no}: bad count line {line!r}")
            counts[int(n)] = int(cnt)
            continue
        fields = line.split()
        n, top = section, section == max(counts)
        if len(fields) not in ((n + 1,) if top else (n + 1, n + 2)):
            raise ValueError(f"read_arpa: line {no}: a {n}-gram line has {n + 1}{'' if top else f' or {n + 2}'} fields, got {len(fields)}: {line!r}")
        try:
            p = float(fields[0])
            bo = float(fields[n + 1]) if len(fields) == n + 2 else 0.0
        except ValueError:
            raise ValueError(f"read_arpa: line {no}: not a number in {line!r}") from None
        if not (math.isfinite(p) or p == -math.inf) or not math.isfinite(bo):
            raise ValueError(f"read_arpa: line {no}: not a finite number in {line!r}")
        gram = tuple(fields[1:n + 1])
        if gram in tables[n]:
            raise ValueError(f"read_arpa: line {no}: the {n}-gram {' '.join(gram)!r} twice")
        tables[n][gram] = (p, bo)
    if not seen_data:
        raise ValueError("read_arpa: line 1: no \\data\\ section")
    if not ended:
        raise ValueError(f"read_arpa: line {len(text.splitlines())}: no \\end\\ marker")
    if not counts:
        raise ValueError("read_arpa: line 1: no `ngram N=count` lines")
    order = max(counts)
    for n in range(1, order + 1):
        if n not in counts or n not in tables:
            raise ValueError(f"read_arpa: line {len(text.splitlines())}: order {n} of {order} is missing")
        if len(tables[n]) != counts[n]:
            raise ValueError(f"read_arpa: line {len(text.splitlines())}: {len(tables[n])} {n}-grams, the \\data\\ section announces {counts[n]}")
    return order, [tables[n] for n in range(1, order + 1)]


@dataclass
class BeamLMResult(BeamResult):
    """`BeamResult` of the fused search (thunder_speech_amd/ctc_beam_lm.h: ts_ctc_beam_lm_search); `scores` are the logs of the fused masses."""
    lm_scores: Any = None     # f32 [B, n_best]         unweighted log10 LM score of the hypothesis, </s> included where it was applied


@dataclass
class LMWeights:
    """Device tables of one (alpha, beta) setting (thunder_speech_amd/ctc_beam_lm.h: ts_ctc_lm); `struct` holds their addresses."""
    alpha: float
    beta: float
    tensors: dict
    struct: object


class NGramLM:
    """A back-off n-gram LM over CTC classes, compiled to an automaton.

    `grams` maps n-grams of ids (classes >= 0, BOS, EOS, UNK) to (log10 p, log10 back-off).  States: the empty context (state 0) and every
    prefix, shorter than the order, of an n-gram -- that is every n-gram of order < N and every context of one --, numbered by (length, ids), so
    that a back-off arc leads to a lower state.  The state after a history is the longest suffix of the history that is a state.  Per state:
    `arcs[s]`, sorted by class, of (class, log10 p, next state = the longest suffix of context + class that is a state), and the back-off arc
    `backoff[s]` = (log10 back-off -- 0 where the context has no line of its own --, the longest proper suffix that is a state).  State 0 has
    an arc for every class but the blank: a class without a unigram takes <unk>'s unigram, or `unk_log10`, and leads to state 0.
    A table that is not prefix-closed (an ARPA file of a toolkit always is) can hold a context + class that is a state without being an
    n-gram; its state then carries an arc with the backed-off log10 p, so that the lookup equals the dictionary back-off for any table."""

    def __init__(self, order: int, grams: Dict[NGram, Tuple[float, float]], n_classes: int, blank_idx: int, unk_log10: float = -10.0, dropped: int = 0):
        self.order, self.n_classes, self.blank_idx, self.unk_log10, self.dropped = int(order), int(n_classes), int(blank_idx), float(unk_log10), int(dropped)
        for g in grams:
            if not 1 <= len(g) <= order or any(c == blank_idx or c >= n_classes or c < UNK for c in g):
                raise ValueError(f"NGramLM: bad n-gram {g}")
        # n-grams the automaton can reach: <s> only in front, </s> only at the end, <unk> only as the unigram
        ok = lambda g: BOS not in g[1:] and EOS not in g[:-1] and (UNK not in g or g == (UNK,))
        self.grams = {g: (float(p), float(bo)) for g, (p, bo) in grams.items() if ok(g)}
        self.has_bos = any(g[0] == BOS for g in self.grams)
        self.has_eos = any(g[-1] == EOS for g in self.grams)
        self.has_unk = (UNK,) in self.grams
        ctx = {g[:k] for g in self.grams for k in range(min(len(g), order - 1) + 1) if k == 0 or g[k - 1] >= 0 or g[k - 1] == BOS}
        self.contexts: List[NGram] = sorted(ctx | {()}, key=lambda c: (len(c), c))
        self.state_id: Dict[NGram, int] = {c: i for i, c in enumerate(self.contexts)}
        self.start_state = self.state_id.get((BOS,), 0)
        self.arcs: List[List[Tuple[int, float, int]]] = [[] for _ in self.contexts]
        self.backoff: List[Tuple[float, int]] = [(self.grams.get(c, (0.0, 0.0))[1], self._suffix_state(c[1:])) if c else (0.0, 0) for c in self.contexts]
        for g, (p, _) in self.grams.items():
            if g[-1] >= 0:
                self.arcs[self.state_id[g[:-1]]].append((g[-1], p, self._suffix_state(g[max(len(g) - order + 1, 0):] if order > 1 else ())))
        for y in self.contexts:
            if y and y[-1] >= 0 and y not in self.grams:                 # a state that is no n-gram: its parent state gets the backed-off arc
                p, floor = self._chain(y[:-1], y[-1])
                if not floor:
                    self.arcs[self.state_id[y[:-1]]].append((y[-1], p, self.state_id[y]))
        have = {a[0] for a in self.arcs[0]}
        self.arcs[0] += [(c, self._chain((), c)[0], 0) for c in range(n_classes) if c != blank_idx and c not in have]
        for a in self.arcs:
            a.sort()
        self.eos_log10 = [self._chain(c, EOS)[0] if self.has_eos else 0.0 for c in self.contexts]
        self._cache: dict = {}

    def _suffix_state(self, c: NGram) -> int:
        while c not in self.state_id:
            c = c[1:]
        return self.state_id[c]

    def _chain(self, c: NGram, w: int) -> Tuple[float, bool]:
        """(log10 P(w | context c), whether it is the floor of a word without a unigram) by the dictionary back-off."""
        total = 0.0
        while True:
            if c + (w,) in self.grams:
                return total + self.grams[c + (w,)][0], False
            if not c:
                return total + (self.grams[(UNK,)][0] if self.has_unk else self.unk_log10), True
            total += self.grams.get(c, (0.0, 0.0))[1]
            c = c[1:]

    @classmethod
    def from_arpa(cls, path: str, itos: Sequence[str], blank_idx: int, token_of: Optional[Callable[[str], str]] = None, unk_log10: float = -10.0) -> "NGramLM":
        """The LM of an ARPA file over the classes `itos`: a word is the class c with itos[c] == word (after `token_of(word)`, if given; the
        first such class); <s>, </s> and <unk> are special, the blank never matches.  N-grams with any other unmatched word are dropped and
        counted in `dropped`."""
        order, tables = read_arpa(path)
        ids: Dict[str, int] = {}
        for c, tok in enumerate(itos):
            if c != blank_idx and tok not in _SPECIAL:
                ids.setdefault(tok, c)
        grams, dropped = {}, 0
        for table in tables:
            for words, val in table.items():
                g = tuple(_SPECIAL[w] if w in _SPECIAL else ids.get(token_of(w) if token_of else w) for w in words)
                if None in g:
                    dropped += 1
                elif g not in grams:
                    grams[g] = val
        return cls(order, grams, len(itos), blank_idx, unk_log10, dropped)

    # ---- lookup on the host (what the kernel does on the device tables) ----
    @property
    def n_states(self) -> int:
        return len(self.contexts)

    def step(self, state: int, c: int) -> Tuple[float, int]:
        """(log10 P(c | state), next state): down the back-off arcs to the first state with an arc of class c."""
        total = 0.0
        while True:
            for cls_, p, nxt in self.arcs[state]:
                if cls_ == c:
                    return total + p, nxt
            if state == 0:
                raise ValueError(f"NGramLM.step: class {c} has no LM id (the blank, or outside the classes)")
            bo, state_next = self.backoff[state]
            total, state = total + bo, state_next
        raise AssertionError

    def eos(self, state: int) -> float:
        return self.eos_log10[state]

    def score(self, labels: Sequence[int], eos: bool = False) -> float:
        """log10 P(labels [</s>]) from the start state."""
        s, total = self.start_state, 0.0
        for c in labels:
            p, s = self.step(s, int(c))
            total += p
        return total + (self.eos(s) if eos and self.has_eos else 0.0)

    # ---- device tables ----
    def tables(self, alpha: float, beta: float) -> Dict[str, np.ndarray]:
        """The numpy tables of ts_ctc_lm for one setting: arc factor 10^(alpha log10 p) e^beta, back-off factor 10^(alpha log10 bo), </s> factor
        10^(alpha log10 P(</s> | state)) (no beta), each one f64 formed here."""
        alpha, beta = float(alpha), float(beta)
        begin = np.zeros(self.n_states + 1, np.int32)
        begin[1:] = np.cumsum([len(a) for a in self.arcs])
        flat = [x for a in self.arcs for x in a]
        arc_log = np.array([x[1] for x in flat], np.float64).reshape(-1)
        bo_log = np.array([b[0] for b in self.backoff], np.float64)
        eos_log = np.array(self.eos_log10, np.float64)
        return {"arc_begin": begin, "arc_class": np.array([x[0] for x in flat], np.int32).reshape(-1),
                "arc_next": np.array([x[2] for x in flat], np.int32).reshape(-1),
                "arc_factor": np.power(10.0, alpha * arc_log) * math.exp(beta), "arc_log10": arc_log,
                "bo_next": np.array([b[1] for b in self.backoff], np.int32), "bo_factor": np.power(10.0, alpha * bo_log), "bo_log10": bo_log,
                "eos_factor": np.power(10.0, alpha * eos_log), "eos_log10": eos_log}

    def weights(self, alpha: float, beta: float, device=None) -> LMWeights:
        """The device tables of one setting, cached per (alpha, beta, device)."""
        import torch
        from . import _lib
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        key = (float(alpha), float(beta), str(dev))
        if key not in self._cache:
            if dev.type != "cuda":
                raise RuntimeError("NGramLM.weights: GPU tensors required (no CPU fallback)")
            t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in self.tables(alpha, beta).items()}
            st = _lib.CtcLm(n_states=self.n_states, n_arcs=int(t["arc_class"].numel()), start_state=self.start_state, has_eos=int(self.has_eos),
                            **{k: v.data_ptr() for k, v in t.items()})
            self._cache[key] = LMWeights(float(alpha), float(beta), t, st)
        return self._cache[key]


def beam_search_lm(logits, lm: NGramLM, alpha: float, beta: float, lengths=None, blank_idx: int = 0, beam_width: int = 16, token_cap: int = 8,
                   n_best: int = 1, score_eos: bool = True):
    """`beam_search` with the n-gram LM fused into the search: score = log(CTC mass of the surviving alignments) + alpha ln 10 log10 P_LM(tokens
    [</s>]) + beta (number of tokens).  Returns a `BeamLMResult`: `BeamResult` extended by `lm_scores` (f32 [B, n_best]: the unweighted log10 LM score)."""
    import ctypes as C
    import torch
    from . import _lib
    from .ctc_align import _logits_f32
    lg = _logits_f32(logits, "beam_search_lm")
    b, v, t = lg.shape
    if b == 0 or t == 0:
        raise ValueError("beam_search_lm: empty logits")
    if not isinstance(lm, NGramLM):
        raise TypeError("beam_search_lm: lm must be an NGramLM")
    if lm.n_classes != v or lm.blank_idx != int(blank_idx):
        raise ValueError(f"beam_search_lm: the LM was compiled for {lm.n_classes} classes with blank {lm.blank_idx}, the logits have {v} with blank {int(blank_idx)}")
    dev = lg.device
    il = None if lengths is None else lengths.to(device=dev, dtype=torch.int64).to(torch.int32).contiguous()
    L = _lib.lib()
    nbytes = L.ts_ctc_beam_lm_workspace_bytes(b, t, int(beam_width), int(token_cap))
    if nbytes < 0:
        _lib.check(int(nbytes), "ts_ctc_beam_lm_workspace_bytes")
    n_best = int(n_best)
    if not 1 <= n_best <= int(beam_width):
        raise ValueError("beam_search_lm: 1 <= n_best <= beam_width required")
    w = lm.weights(alpha, beta, dev)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    tokens = torch.empty(b, n_best, t, dtype=torch.int32, device=dev)
    frames = torch.empty(b, n_best, t, dtype=torch.int32, device=dev)
    out_len = torch.empty(b, n_best, dtype=torch.int32, device=dev)
    scores = torch.empty(b, n_best, dtype=torch.float32, device=dev)
    lm_scores = torch.empty(b, n_best, dtype=torch.float32, device=dev)
    counts = torch.empty(b, dtype=torch.int32, device=dev)
    st = L.ts_ctc_beam_lm_search(lg.data_ptr(), b, v, t, lg.stride(1), None if il is None else il.data_ptr(), int(blank_idx), int(beam_width),
                                 int(token_cap), n_best, int(bool(score_eos)), C.byref(w.struct), tokens.data_ptr(), frames.data_ptr(),
                                 out_len.data_ptr(), scores.data_ptr(), lm_scores.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                 torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(st, "ts_ctc_beam_lm_search")
    return BeamLMResult(tokens, frames, out_len, scores, counts, lm_scores)


# ---- word-level LM over a character vocabulary: lexicon trie, hot words (thunder_speech_amd/ctc_beam_word_lm.h) ---------------------------------
class WordStep(NamedTuple):
    """What one class does to the pair (word state, lexicon state) on the host: the unweighted log10 met, the pair entered, whether the OOV
    factor is paid here (a `PieceWordNGramLM` counts how often: a piece can end one word and leave the trie with the next), and the lexicon word that ended here (None: none, or a word outside the lexicon)."""
    log10: float
    state: int
    x: int
    oov: bool
    word: Optional[int]


@dataclass
class WordLMWeights:
    """Device tables of one (alpha, beta, oov_score, boosts) setting: `lm` the word automaton's (LMWeights), `struct` the ts_ctc_lexicon."""
    lm: LMWeights
    oov_score: float
    boosts: Tuple[float, ...]
    tensors: dict
    struct: object


class _WordLM:
    """What the word-level LMs share: the host walk over (word state, lexicon state) pairs and the lexicon tables of a setting.  A subclass
    provides `lm`, `words`, `hot`, `word_class`, `unk_class`, `edges`, `node_word` and `step`."""

    def _compile(self, order: int, grams: Dict[Tuple[str, ...], Tuple[float, float]], spelled: Callable[[str], Optional[Tuple[int, ...]]],
                 unspellable: set, lexicon, hotwords, unk_log10: float) -> None:
        """The word automaton and the trie of the words that `spelled` can write (it returns None for the others and notes them in
        `unspellable`); the trie's edges carry what `spelled` returns: CTC classes, or letter ids."""
        # the word automaton: the existing machinery, with word ids as classes
        lm_words = sorted({w for g in grams for w in g if w not in _SPECIAL})
        self.lm_words: List[str] = [w for w in lm_words if spelled(w) is not None]
        lm_id = {w: i for i, w in enumerate(self.lm_words)}
        self.unk_class = len(self.lm_words)
        id_grams, self.dropped_ngrams = {}, 0
        for g, val in grams.items():
            ids = tuple(_SPECIAL[w] if w in _SPECIAL else lm_id.get(w) for w in g)
            if None in ids:
                self.dropped_ngrams += 1
            else:
                id_grams.setdefault(ids, val)
        self.order = int(order)
        self.lm = NGramLM(order, id_grams, self.unk_class + 2, self.unk_class + 1, unk_log10, self.dropped_ngrams)
        # the lexicon: the given words (default: the LM's spellable unigrams) and the hot words
        hot = set(hotwords)
        listed = [w for w in self.lm_words if (w,) in grams] if lexicon is None else list(lexicon)
        spellings = {w: spelled(w) for w in sorted(set(listed) | hot) if w not in _SPECIAL}
        self.words: List[str] = [w for w, sp in spellings.items() if sp is not None]
        self.spellings: List[Tuple[int, ...]] = [spellings[w] for w in self.words]
        self.hot: List[bool] = [w in hot for w in self.words]
        self.word_class: List[int] = [lm_id.get(w, self.unk_class) for w in self.words]
        self.dropped = len(unspellable)
        prefixes = sorted({sp[:k] for sp in self.spellings for k in range(len(sp) + 1)} | {()}, key=lambda p: (len(p), p))
        self.node_id: Dict[Tuple[int, ...], int] = {p: i for i, p in enumerate(prefixes)}
        self.edges: List[List[Tuple[int, int]]] = [[] for _ in prefixes]
        for p in prefixes[1:]:
            self.edges[self.node_id[p[:-1]]].append((p[-1], self.node_id[p]))
        for e in self.edges:
            e.sort()
        self.node_word: List[int] = [-1] * len(prefixes)
        for w, sp in enumerate(self.spellings):
            if self.node_word[self.node_id[sp]] < 0:
                self.node_word[self.node_id[sp]] = w
        self._static: dict = {}
        self._cache: dict = {}

    # ---- lookup on the host (what the kernel does on the device tables) ----
    @property
    def n_nodes(self) -> int:
        return len(self.node_word)

    @property
    def start_state(self) -> int:
        return self.lm.start_state

    def finish(self, state: int, x: int) -> WordStep:
        """The end of the pending word, as if a word boundary followed; nothing happens at the root."""
        if x == 0:
            return WordStep(0.0, state, 0, False, None)
        w = self.node_word[x] if x > 0 else -1
        p, nxt = self.lm.step(state, self.word_class[w] if w >= 0 else self.unk_class)
        return WordStep(p, nxt, 0, w < 0 and x > 0, w if w >= 0 else None)

    def walk(self, labels: Sequence[int], eos: bool = False) -> Tuple[float, int, List[int]]:
        """(log10 P(words [</s>]), OOV words, lexicon words in order) of a label string from the start, the pending word included."""
        s, x, total, oov, words = self.start_state, 0, 0.0, 0, []
        for k in range(len(labels) + 1):
            r = self.step(s, x, labels[k]) if k < len(labels) else self.finish(s, x)
            total, s, x, oov = total + r.log10, r.state, r.x, oov + int(r.oov)
            if r.word is not None:
                words.append(r.word)
        return total + (self.lm.eos(s) if eos and self.lm.has_eos else 0.0), oov, words

    def score(self, labels: Sequence[int], eos: bool = False) -> float:
        """log10 P(the words of labels [</s>]) from the start state: a word outside the lexicon is <unk>; the pending word counts."""
        return self.walk(labels, eos)[0]

    # ---- device tables ----
    def word_boosts(self, hotword_weight: float = 0.0, boosts: Optional[Dict[str, float]] = None) -> Tuple[float, ...]:
        """The boost of every lexicon word: `boosts[word]` where given, else `hotword_weight` for a hot word, else 0."""
        boosts = dict(boosts or {})
        unknown = [w for w in boosts if w not in self.words or not self.hot[self.words.index(w)]]
        if unknown:
            raise ValueError(f"{type(self).__name__}: boosts for {unknown}, which are not hot words of this LM")
        return tuple(float(boosts.get(w, hotword_weight)) if h else 0.0 for w, h in zip(self.words, self.hot))

    def lexicon_tables(self, oov_score: float = -10.0, hotword_weight: float = 0.0, boosts: Optional[Dict[str, float]] = None) -> Dict[str, np.ndarray]:
        """The numpy tables of ts_ctc_lexicon for one setting: oov_factor = e^oov_score, word_factor = e^boost (1 for a word that is not hot),
        each one f64 formed here."""
        begin = np.zeros(self.n_nodes + 1, np.int32)
        begin[1:] = np.cumsum([len(e) for e in self.edges])
        flat = [x for e in self.edges for x in e]
        return {"edge_begin": begin, "edge_class": np.array([x[0] for x in flat], np.int32).reshape(-1),
                "edge_next": np.array([x[1] for x in flat], np.int32).reshape(-1), "node_word": np.array(self.node_word, np.int32),
                "word_class": np.array(self.word_class, np.int32).reshape(-1),
                "word_factor": np.exp(np.array(self.word_boosts(hotword_weight, boosts), np.float64)).reshape(-1),
                "oov_factor": np.exp(np.array([float(oov_score)], np.float64))}


class WordNGramLM(_WordLM):
    """A word-level back-off n-gram LM for a CHARACTER vocabulary, with the lexicon trie that spells its words in CTC classes.

    `words` are the lexicon's words in trie order, `spellings[w]` the classes of word w, `hot[w]` whether it is a hot word, `word_class[w]` its
    class in the word automaton `lm` -- an `NGramLM` whose classes are the ids of the LM's spellable words (`lm_words`), then `unk_class` for
    <unk>-as-a-word (a lexicon word the LM lacks has that class), then a class that plays the blank and is never looked up.  Trie: node 0 is the
    root, `edges[x]` the (class, next node) pairs of node x sorted by class, `node_word[x]` the word that ends at x or -1.  Two words with one
    spelling share a node; the first in sorted order is the node's word."""

    def __init__(self, order: int, grams: Dict[Tuple[str, ...], Tuple[float, float]], itos: Sequence[str], blank_idx: int, delimiter: str = " ",
                 lexicon=None, hotwords=(), spell: Optional[Callable[[str], str]] = None, unk_log10: float = -10.0):
        self.n_classes, self.blank_idx = len(itos), int(blank_idx)
        where = [c for c, tok in enumerate(itos) if tok == delimiter and c != self.blank_idx]
        if not where:
            raise ValueError(f"WordNGramLM: the vocabulary has no class {delimiter!r} to end a word")
        self.delimiter = where[0]
        letters: Dict[str, int] = {}
        for c, tok in enumerate(itos):
            if c not in (self.blank_idx, self.delimiter) and tok not in _SPECIAL and len(tok) == 1:
                letters.setdefault(tok, c)
        unspellable = set()

        def spelled(word: str) -> Optional[Tuple[int, ...]]:
            text = spell(word) if spell else word
            if not text or any(ch not in letters for ch in text):
                unspellable.add(word)
                return None
            return tuple(letters[ch] for ch in text)

        self._compile(order, grams, spelled, unspellable, lexicon, hotwords, unk_log10)

    @classmethod
    def from_arpa(cls, path: str, itos: Sequence[str], blank_idx: int, delimiter: str = " ", lexicon=None, hotwords=(),
                  spell: Optional[Callable[[str], str]] = None, unk_log10: float = -10.0) -> "WordNGramLM":
        """The word LM of an ARPA file over the character classes `itos`.  A word is kept if `spell(word)` (default: the word itself) can be
        written in the one-character classes without the blank and without the class `delimiter`; n-grams with another word are dropped.
        `lexicon` (an iterable of words; default: the LM's spellable unigrams) and `hotwords` form the trie; a word of either that the LM lacks
        is scored as <unk>.  `dropped` counts the words -- of the file, the lexicon or the hot words -- that cannot be spelled."""
        order, tables = read_arpa(path)
        return cls(order, {g: v for t in tables for g, v in t.items()}, itos, blank_idx, delimiter, lexicon, hotwords, spell, unk_log10)

    # ---- lookup on the host (what the kernel does on the device tables) ----
    def step(self, state: int, x: int, c: int) -> WordStep:
        """Class c (neither the blank nor outside the classes) from the pair (state, x)."""
        c = int(c)
        if c == self.blank_idx or not 0 <= c < self.n_classes:
            raise ValueError(f"WordNGramLM.step: class {c} is the blank, or outside the classes")
        if c == self.delimiter:
            return self.finish(state, x)
        if x < 0:
            return WordStep(0.0, state, -1, False, None)
        for cls_, nxt in self.edges[x]:
            if cls_ == c:
                return WordStep(0.0, state, nxt, False, None)
        return WordStep(0.0, state, -1, True, None)

    # ---- device tables ----
    def weights(self, alpha: float, beta: float, oov_score: float = -10.0, hotword_weight: float = 0.0, boosts: Optional[Dict[str, float]] = None,
                device=None) -> WordLMWeights:
        """The device tables of one setting, cached per (alpha, beta, oov_score, boosts of the words, device).  A NEW setting gets NEW
        word_factor / oov_factor tensors (and, for a new (alpha, beta), new factor tables of the word automaton): nothing is written at the
        addresses of another setting, so a graph captured under the old setting keeps replaying the old setting.  The trie's tables do not
        depend on the setting and are shared per device."""
        import torch
        from . import _lib
        per_word = self.word_boosts(hotword_weight, boosts)
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("WordNGramLM.weights: GPU tensors required (no CPU fallback)")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        key = (float(alpha), float(beta), float(oov_score), per_word, str(dev))
        if key not in self._cache:
            up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
            tables = self.lexicon_tables(oov_score, hotword_weight, boosts)
            if str(dev) not in self._static:
                self._static[str(dev)] = {k: up(tables[k]) for k in ("edge_begin", "edge_class", "edge_next", "node_word", "word_class")}
            t = dict(self._static[str(dev)], word_factor=up(tables["word_factor"]), oov_factor=up(tables["oov_factor"]))
            st = _lib.CtcLexicon(n_nodes=self.n_nodes, n_edges=int(t["edge_class"].numel()), n_words=len(self.words), delimiter=self.delimiter,
                                 unk_class=self.unk_class, **{k: v.data_ptr() for k, v in t.items()})
            self._cache[key] = WordLMWeights(self.lm.weights(alpha, beta, dev), float(oov_score), per_word, t, st)
        return self._cache[key]


def beam_search_word_lm(logits, lm: WordNGramLM, alpha: float, beta: float, lengths=None, blank_idx: int = 0, beam_width: int = 16,
                        token_cap: int = 8, n_best: int = 1, score_eos: bool = True, oov_score: float = -10.0, hotword_weight: float = 0.0,
                        boosts: Optional[Dict[str, float]] = None):
    """`beam_search` over a character vocabulary with the word-level n-gram LM, its lexicon and its hot words fused into the search
    (csrc/ctc_beam_word_lm.hip): score = log(CTC mass of the surviving alignments) + alpha ln 10 log10 P_LM(words [</s>]) + beta (number of
    words) + oov_score (number of words outside the lexicon) + the boosts of the hot words; the word that the clip ends in counts.  Returns a
    `BeamLMResult`; `lm_scores` is the unweighted log10 LM score of the words."""
    import ctypes as C
    import torch
    from . import _lib
    from .ctc_align import _logits_f32
    lg = _logits_f32(logits, "beam_search_word_lm")
    b, v, t = lg.shape
    if b == 0 or t == 0:
        raise ValueError("beam_search_word_lm: empty logits")
    if not isinstance(lm, WordNGramLM):
        raise TypeError("beam_search_word_lm: lm must be a WordNGramLM")
    if lm.n_classes != v or lm.blank_idx != int(blank_idx):
        raise ValueError(f"beam_search_word_lm: the LM was compiled for {lm.n_classes} classes with blank {lm.blank_idx}, the logits have {v} with blank {int(blank_idx)}")
    dev = lg.device
    il = None if lengths is None else lengths.to(device=dev, dtype=torch.int64).to(torch.int32).contiguous()
    L = _lib.lib()
    nbytes = L.ts_ctc_beam_word_lm_workspace_bytes(b, t, int(beam_width), int(token_cap))
    if nbytes < 0:
        _lib.check(int(nbytes), "ts_ctc_beam_word_lm_workspace_bytes")
    n_best = int(n_best)
    if not 1 <= n_best <= int(beam_width):
        raise ValueError("beam_search_word_lm: 1 <= n_best <= beam_width required")
    w = lm.weights(alpha, beta, oov_score, hotword_weight, boosts, dev)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    tokens = torch.empty(b, n_best, t, dtype=torch.int32, device=dev)
    frames = torch.empty(b, n_best, t, dtype=torch.int32, device=dev)
    out_len = torch.empty(b, n_best, dtype=torch.int32, device=dev)
    scores = torch.empty(b, n_best, dtype=torch.float32, device=dev)
    lm_scores = torch.empty(b, n_best, dtype=torch.float32, device=dev)
    counts = torch.empty(b, dtype=torch.int32, device=dev)
    st = L.ts_ctc_beam_word_lm_search(lg.data_ptr(), b, v, t, lg.stride(1), None if il is None else il.data_ptr(), int(blank_idx), int(beam_width),
                                      int(token_cap), n_best, int(bool(score_eos)), C.byref(w.lm.struct), C.byref(w.struct), tokens.data_ptr(),
                                      frames.data_ptr(), out_len.data_ptr(), scores.data_ptr(), lm_scores.data_ptr(), counts.data_ptr(),
                                      ws.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(st, "ts_ctc_beam_word_lm_search")
    return BeamLMResult(tokens, frames, out_len, scores, counts, lm_scores)


# ---- word-level LM over a sentencepiece vocabulary: a trie over letters, pieces that start words (thunder_speech_amd/ctc_beam_piece_lm.h) -------
@dataclass
class PieceLMWeights(WordLMWeights):
    """`WordLMWeights` of a `PieceWordNGramLM`: `struct` is the ts_ctc_lexicon over letters, `pieces` the ts_ctc_pieces (its tensors are in
    `tensors` too)."""
    pieces: object = None


class PieceWordNGramLM(_WordLM):
    """A word-level back-off n-gram LM for a SENTENCEPIECE vocabulary, with the lexicon trie that spells its words in letters.

    A class whose token begins with `word_start` starts a word (kind 1), any other continues one (kind 0); a LETTER is a character of some such
    token once the leading `word_start` is stripped, and `letters` lists them in sorted order: their positions are the letter ids.
    `piece_letters[c]` are the letter ids of class c (none for a bare `word_start`) and `piece_kind[c]` its kind.  A class whose token is <s>,
    </s> or <unk>, or holds `word_start` anywhere but at the front, has no spelling (kind 2; `unspellable_classes` lists them): inside a word
    it makes the word OOV.  The trie's edges carry letter ids, so every segmentation of a word reaches the same node.  `words`, `hot`,
    `word_class`, `lm`, `lm_words`, `unk_class`, `edges`, `node_word`, `dropped` and `dropped_ngrams` are those of `WordNGramLM`."""

    def __init__(self, order: int, grams: Dict[Tuple[str, ...], Tuple[float, float]], itos: Sequence[str], blank_idx: int, word_start: str = "▁",
                 lexicon=None, hotwords=(), spell: Optional[Callable[[str], str]] = None, unk_log10: float = -10.0):
        if not word_start:
            raise ValueError("PieceWordNGramLM: word_start is empty")
        self.itos, self.n_classes, self.blank_idx, self.word_start = list(itos), len(itos), int(blank_idx), word_start
        if not 0 <= self.blank_idx < self.n_classes:
            raise ValueError(f"PieceWordNGramLM: the blank {blank_idx} is outside the {self.n_classes} classes")
        body = lambda tok: tok[len(word_start):] if tok.startswith(word_start) else tok
        self.piece_kind: List[int] = [0 if c == self.blank_idx else 2 if tok in _SPECIAL or word_start in body(tok) else int(tok.startswith(word_start))
                                      for c, tok in enumerate(self.itos)]
        self.unspellable_classes: List[int] = [c for c, k in enumerate(self.piece_kind) if k == 2]
        spellable = {c for c, k in enumerate(self.piece_kind) if k != 2 and c != self.blank_idx}
        self.letters: List[str] = sorted({ch for c in spellable for ch in body(self.itos[c])})
        letter_id = {ch: i for i, ch in enumerate(self.letters)}
        self.piece_letters: List[Tuple[int, ...]] = [tuple(letter_id[ch] for ch in body(tok)) if c in spellable else () for c, tok in enumerate(self.itos)]
        unspellable = set()

        def spelled(word: str) -> Optional[Tuple[int, ...]]:
            text = spell(word) if spell else word
            if not text or any(ch not in letter_id for ch in text):
                unspellable.add(word)
                return None
            return tuple(letter_id[ch] for ch in text)

        self._compile(order, grams, spelled, unspellable, lexicon, hotwords, unk_log10)

    @classmethod
    def from_arpa(cls, path: str, itos: Sequence[str], blank_idx: int, word_start: str = "▁", lexicon=None, hotwords=(),
                  spell: Optional[Callable[[str], str]] = None, unk_log10: float = -10.0) -> "PieceWordNGramLM":
        """The word LM of an ordinary word-level ARPA file over the sentencepiece classes `itos`.  A word is kept if `spell(word)` (default: the
        word itself) can be written in the letters of the pieces; n-grams with another word are dropped.  `lexicon`, `hotwords`, `unk_log10`
        and `dropped` are those of `WordNGramLM.from_arpa`."""
        order, tables = read_arpa(path)
        return cls(order, {g: v for t in tables for g, v in t.items()}, itos, blank_idx, word_start, lexicon, hotwords, spell, unk_log10)

    # ---- lookup on the host (what the kernel does on the device tables) ----
    def step(self, state: int, x: int, c: int) -> WordStep:
        """Class c (neither the blank nor outside the classes) from the pair (state, x): a piece that starts a word ends the pending one, then
        its letters walk the trie.  `oov` COUNTS the OOV factors paid here: the word that ended at a node that is no word, and the word that the
        piece's letters (or a class without a spelling) take out of the trie -- 0, 1 or 2."""
        c = int(c)
        if c == self.blank_idx or not 0 <= c < self.n_classes:
            raise ValueError(f"PieceWordNGramLM.step: class {c} is the blank, or outside the classes")
        kind, log10, oov, word = self.piece_kind[c], 0.0, 0, None
        if kind == 1 and x != 0:
            log10, state, x, ended_oov, word = self.finish(state, x)
            oov += int(ended_oov)
        for letter in self.piece_letters[c] if kind != 2 else (-1,):           # a class without a spelling: one letter that no node has an edge for
            if x < 0:
                break
            nxt = [n for cls_, n in self.edges[x] if cls_ == letter]
            x, oov = (nxt[0], oov) if nxt else (-1, oov + 1)
        return WordStep(log10, state, x, oov, word)

    # ---- device tables ----
    def piece_tables(self) -> Dict[str, np.ndarray]:
        """The numpy tables of ts_ctc_pieces: piece_begin [n_classes + 1], piece_letter, piece_kind [n_classes]."""
        begin = np.zeros(self.n_classes + 1, np.int32)
        begin[1:] = np.cumsum([len(p) for p in self.piece_letters])
        return {"piece_begin": begin, "piece_letter": np.array([x for p in self.piece_letters for x in p], np.int32).reshape(-1),
                "piece_kind": np.array(self.piece_kind, np.int32)}

    def weights(self, alpha: float, beta: float, oov_score: float = -10.0, hotword_weight: float = 0.0, boosts: Optional[Dict[str, float]] = None,
                device=None) -> PieceLMWeights:
        """The device tables of one setting, with the cache and the fixed-address rules of `WordNGramLM.weights`: a NEW setting gets NEW
        word_factor / oov_factor tensors, so a graph captured under the old setting keeps replaying it; the trie's and the pieces' tables do
        not depend on the setting and are shared per device."""
        import torch
        from . import _lib
        per_word = self.word_boosts(hotword_weight, boosts)
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("PieceWordNGramLM.weights: GPU tensors required (no CPU fallback)")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        key = (float(alpha), float(beta), float(oov_score), per_word, str(dev))
        if key not in self._cache:
            up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
            tables = self.lexicon_tables(oov_score, hotword_weight, boosts)
            if str(dev) not in self._static:
                self._static[str(dev)] = ({k: up(tables[k]) for k in ("edge_begin", "edge_class", "edge_next", "node_word", "word_class")},
                                          {k: up(v) for k, v in self.piece_tables().items()})
            trie, pieces = self._static[str(dev)]
            t = dict(trie, word_factor=up(tables["word_factor"]), oov_factor=up(tables["oov_factor"]))
            st = _lib.CtcLexicon(n_nodes=self.n_nodes, n_edges=int(t["edge_class"].numel()), n_words=len(self.words), delimiter=-1,
                                 unk_class=self.unk_class, **{k: v.data_ptr() for k, v in t.items()})
            pc = _lib.CtcPieces(n_classes=self.n_classes, n_letters=len(self.letters), n_piece_letters=int(pieces["piece_letter"].numel()),
                                **{k: v.data_ptr() for k, v in pieces.items()})
            self._cache[key] = PieceLMWeights(self.lm.weights(alpha, beta, dev), float(oov_score), per_word, dict(t, **pieces), st, pc)
        return self._cache[key]


def beam_search_piece_lm(logits, lm: PieceWordNGramLM, alpha: float, beta: float, lengths=None, blank_idx: int = 0, beam_width: int = 16,
                         token_cap: int = 8, n_best: int = 1, score_eos: bool = True, oov_score: float = -10.0, hotword_weight: float = 0.0,
                         boosts: Optional[Dict[str, float]] = None):
    """`beam_search_word_lm` for a sentencepiece vocabulary (csrc/ctc_beam_piece_lm.hip): a word ends where a piece that starts the next one
    follows, and at the end of the clip; score = log(CTC mass of the surviving alignments) + alpha ln 10 log10 P_LM(words [</s>]) + beta
    (number of words) + oov_score (number of words outside the lexicon) + the boosts of the hot words.  Hypotheses are sequences of pieces: two
    segmentations of one text are two hypotheses.  Returns a `BeamLMResult`; `lm_scores` is the unweighted log10 LM score of the words."""
    import ctypes as C
    import torch
    from . import _lib
    from .ctc_align import _logits_f32
    lg = _logits_f32(logits, "beam_search_piece_lm")
    b, v, t = lg.shape
    if b == 0 or t == 0:
        raise ValueError("beam_search_piece_lm: empty logits")
    if not isinstance(lm, PieceWordNGramLM):
        raise TypeError("beam_search_piece_lm: lm must be a PieceWordNGramLM")
    if lm.n_classes != v or lm.blank_idx != int(blank_idx):
        raise ValueError(f"beam_search_piece_lm: the LM was compiled for {lm.n_classes} classes with blank {lm.blank_idx}, the logits have {v} with blank {int(blank_idx)}")
    dev = lg.device
    il = None if lengths is None else lengths.to(device=dev, dtype=torch.int64).to(torch.int32).contiguous()
    L = _lib.lib()
    nbytes = L.ts_ctc_beam_piece_lm_workspace_bytes(b, t, int(beam_width), int(token_cap))
    if nbytes < 0:
        _lib.check(int(nbytes), "ts_ctc_beam_piece_lm_workspace_bytes")
    n_best = int(n_best)
    if not 1 <= n_best <= int(beam_width):
        raise ValueError("beam_search_piece_lm: 1 <= n_best <= beam_width required")
    w = lm.weights(alpha, beta, oov_score, hotword_weight, boosts, dev)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    tokens = torch.empty(b, n_best, t, dtype=torch.int32, device=dev)
    frames = torch.empty(b, n_best, t, dtype=torch.int32, device=dev)
    out_len = torch.empty(b, n_best, dtype=torch.int32, device=dev)
    scores = torch.empty(b, n_best, dtype=torch.float32, device=dev)
    lm_scores = torch.empty(b, n_best, dtype=torch.float32, device=dev)
    counts = torch.empty(b, dtype=torch.int32, device=dev)
    st = L.ts_ctc_beam_piece_lm_search(lg.data_ptr(), b, v, t, lg.stride(1), None if il is None else il.data_ptr(), int(blank_idx), int(beam_width),
                                       int(token_cap), n_best, int(bool(score_eos)), C.byref(w.lm.struct), C.byref(w.struct), C.byref(w.pieces),
                                       tokens.data_ptr(), frames.data_ptr(), out_len.data_ptr(), scores.data_ptr(), lm_scores.data_ptr(),
                                       counts.data_ptr(), ws.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(st, "ts_ctc_beam_piece_lm_search")
    return BeamLMResult(tokens, frames, out_len, scores, counts, lm_scores)
