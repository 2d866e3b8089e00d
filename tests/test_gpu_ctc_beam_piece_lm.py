"""CTC prefix beam search over a sentencepiece vocabulary with a word-level n-gram LM, a lexicon and hot words on the GPU
(include_open/thunder_speech_amd/ctc_beam_piece_lm.h, csrc/ctc_beam_piece_lm.hip) through the raw C ABI and through the module.

The reference is `_search_piece` below: the header's algorithm restated in float64 in the LOG domain, in the style of `_search_word` of
tests/test_gpu_ctc_beam_word_lm.py, with prefixes as tuples of classes (no hashes, no trie, no automaton, no letter ids).  It knows only STRINGS:
the text of a prefix is its pieces joined (a class without a spelling writes "?", which is no letter), the pending word is what follows the last
U+2581 of the text, the lexicon is a plain set of strings (and "can a spelling of the lexicon begin so" a set of strings too), and the LM score of
a word is read from the n-gram DICTIONARY by the textbook back-off (`_textbook`), the context being the words so far (emptied by a word that took
the floor).  Nothing of the package takes part in it.  Independent of that restatement, the exhaustive case compares every score with CTC
log-likelihood (plain float64 alpha recursion) + alpha ln 10 LM(words) + beta (words) + oov_score (OOV words) + boosts (+ </s>), the words found
by replacing U+2581 by a space in the text and splitting.

Tolerance of a score and of an lm_score: 2^-23 max(1, |value|) -- the one f32 rounding (2^-24 relative) plus float64 noise.

The margin condition (asserted by every test that demands equal tokens) is that of tests/test_gpu_ctc_beam_word_lm.py, re-derived for the new
child rule.  The token-level count of tests/test_gpu_ctc_beam_lm.py per frame and side is fewer than 32 + 4 N + 4 ulp (N the LM's order; the
lookup of the word that a child ends is in it).  On top of it a child can now meet TWO more products on the device: the factor of the word it ends
(word_factor, or oov_factor at a node that is no word) and one oov_factor for the word it begins, where its letters -- however many -- leave the
trie: the walk over the letters pays at most once, and a letter that follows an edge costs no arithmetic.  Each is one f64 product by a factor
that carries up to 2 ulp of its own (one exponential on the host): 6 ulp relative, the two products the sibling's bound already counts (there a
child meets one of them; the count was taken for both).  In the reference the matching sums -- the boost or the OOV score of the word ended, the OOV
score of the word begun, and the sum of the two -- are at most 3 roundings, each an absolute error of an ulp of the magnitude of its partial sum, at
most max(M, L), M the largest |log key| and L the largest |weight of a child| (alpha ln 10 log10 p + beta + boost + the OOV scores): 3 <= 6.
Fewer than 32 + 4 N + 4 + 6 <= 40 + 8 N ulp per frame on either side.  The pending word after the last frame is one more such step (and the one
</s> product is covered by the slack of the first term), so the errors add up linearly over T + 1 steps: two log keys closer than
E = (80 + 16 N) (T + 1) 2^-53 max(1, M, L) may fall either way, and the tests require the smallest gap (last kept key against first dropped key
over all frames, and neighbouring keys of the final beam after the pending words and </s>) to exceed E.  The fixtures' margins were measured on
the CPU before the seeds were fixed (>= 2e-3 against E <= 5e-11); the assertion stays in every test.

Ratios error / bound are printed as `RATIO|kind|ratio|case`."""
import functools
import math
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARPA = os.path.join(ROOT, "tests", "golden", "lm_words_tiny.arpa")
NEG = float("-inf")
U53 = 2.0 ** -53
LN10 = math.log(10.0)
BOS, EOS, UNK = "<s>", "</s>", "<unk>"
UNKW = "a word the LM does not know"                                         # what such a word is looked up as: in no n-gram
FLOOR = -4.0                                                                 # log10 p of a word without a unigram in an LM without <unk>
WS = "▁"


def _tol(v):
    return 2.0 ** -23 * max(1.0, abs(v))


# ---- the reference -------------------------------------------------------------------------------------------------------------------------------
def _ladd(a, b):
    if a == NEG:
        return b
    if b == NEG:
        return a
    return max(a, b) + math.log1p(math.exp(-abs(a - b)))


def _log_softmax64(x):
    x = x.astype(np.float64)
    m = x.max(0, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(0, keepdims=True)))


def _textbook(grams, order, hist, w):
    """(log10 P(w | hist), fell to the floor) by the dictionary back-off: the n-gram if the table has it, else back-off(context) + the same with a
    shorter context; a word without a unigram takes <unk>'s unigram or the floor."""
    total = 0.0
    ctx = tuple(hist[max(len(hist) - (order - 1), 0):]) if order > 1 else ()
    while True:
        if ctx + (w,) in grams:
            return total + grams[ctx + (w,)][0], False
        if not ctx:
            return total + (grams[(UNK,)][0] if (UNK,) in grams else FLOOR), True
        total += grams.get(ctx, (0.0, 0.0))[1]
        ctx = ctx[1:]


class _Strings:
    """What the reference knows: the classes' tokens, the n-gram dictionary over word strings, the lexicon as a set of strings, the boost of each
    hot word, and the four weights."""

    def __init__(self, itos, blank, grams, order, lexicon, hot, alpha, beta, oov_score):
        self.itos, self.blank, self.grams, self.order, self.lexicon, self.hot = list(itos), blank, grams, order, set(lexicon), dict(hot)
        self.alpha, self.beta, self.oov_score = alpha, beta, oov_score
        self.begins = {w[:k] for w in self.lexicon for k in range(len(w) + 1)} | {""}           # what a spelling of the lexicon can begin with
        self.known = {w for g in grams for w in g if w not in (BOS, EOS, UNK)}                  # the LM's words
        self.has_eos = any(g[-1] == EOS for g in grams)
        self.start = (BOS,) if any(g[0] == BOS for g in grams) else ()

    def piece(self, c):
        """What class c writes: its token, or "?" -- no letter -- for a class without a spelling."""
        tok = self.itos[c]
        return "?" if tok in (BOS, EOS, UNK) or WS in tok[1:] else tok

    def text(self, pre):
        return "".join(self.piece(c) for c in pre)

    def pending(self, pre):
        """What follows the last word start of a prefix's text."""
        return self.text(pre).split(WS)[-1]

    def end_word(self, cur, hist):
        """(log weight, log10 LM score, context after) of the word `cur` ending in the context `hist`."""
        if cur in self.lexicon:
            key, extra = (cur if cur in self.known else UNKW), self.hot.get(cur, 0.0)
        else:
            key, extra = UNKW, (self.oov_score if cur in self.begins else 0.0)                  # a spelling that left the lexicon paid when it left
        lp, fell = _textbook(self.grams, self.order, hist, key)
        return self.alpha * LN10 * lp + self.beta + extra, lp, (() if fell else hist + (key,))

    def child(self, pre, hist, c):
        """(log weight, log10 LM score, context after) of class c after the prefix `pre` whose words so far are `hist`."""
        cur, p, w, lp = self.pending(pre), self.piece(c), 0.0, 0.0
        if p.startswith(WS):
            if cur:
                w, lp, hist = self.end_word(cur, hist)
            cur, p = "", p[1:]
        if cur in self.begins and cur + p not in self.begins:                # the spelling leaves the lexicon within this piece: once
            w = w + self.oov_score
        return w, lp, hist


def _search_piece(x, width, cap, k, eos):
    """x [V, T] f32, k a _Strings -> (final beam [(prefix, frames, log key, log10 LM score)], smallest decision gap, largest magnitude): the header,
    word by word."""
    V, T = x.shape
    blank = k.blank
    cap = min(cap, V - 1)
    beam = [((), (), 0.0, NEG, k.start, 0.0)]                              # prefix, frames, p_b, p_nb, LM context, log10 LM score so far
    gap, big = math.inf, 0.0
    for t in range(T):
        p = _log_softmax64(x[:, t:t + 1])[:, 0]
        cands = sorted(sorted((c for c in range(V) if c != blank), key=lambda c: (-float(x[c, t]), c))[:cap])     # raw logits; ascending class order
        slot = {e[0]: j for j, e in enumerate(beam)}
        stay = [[_ladd(pb, pnb) + p[blank], pnb + p[pre[-1]] if pre else NEG] for pre, _, pb, pnb, _, _ in beam]
        children = []
        for pre, fr, pb, pnb, hist, lm10 in beam:                          # children in (parent slot, class index) order
            tot = _ladd(pb, pnb)
            for c in cands:
                w, lp, nhist = k.child(pre, hist, c)
                big = max(big, abs(w))
                mass = (pb if pre and pre[-1] == c else tot) + p[c] + w
                if pre + (c,) in slot:
                    j = slot[pre + (c,)]
                    stay[j][1] = _ladd(stay[j][1], mass)
                else:
                    children.append((pre + (c,), fr + (t,), NEG, mass, nhist, lm10 + lp))
        allc = [(e[0], e[1], s[0], s[1], e[4], e[5]) for e, s in zip(beam, stay)] + children
        keys = [_ladd(c[2], c[3]) for c in allc]
        order_ = [j for j in sorted(range(len(allc)), key=lambda j: (-keys[j], j)) if keys[j] != NEG]
        if len(order_) > width:
            gap = min(gap, keys[order_[width - 1]] - keys[order_[width]])
        beam = [allc[j] for j in order_[:width]]
        big = max([big] + [abs(keys[j]) for j in order_[:width]])
    final = []
    for pre, fr, pb, pnb, hist, lm10 in beam:
        key, end10 = _ladd(pb, pnb), 0.0
        cur = k.pending(pre)
        if cur:                                                             # the pending word, whatever eos says
            w, lp, hist = k.end_word(cur, hist)
            key, end10 = key + w, end10 + lp
            big = max(big, abs(w), abs(key))
        if eos and k.has_eos:
            lp = _textbook(k.grams, k.order, hist, EOS)[0]
            key, end10 = key + k.alpha * LN10 * lp, end10 + lp
            big = max(big, abs(k.alpha * LN10 * lp), abs(key))
        final.append((pre, fr, key, lm10 + end10))
    final = [final[j] for j in sorted(range(len(final)), key=lambda j: (-final[j][2], j))]
    for a, b in zip(final, final[1:]):
        gap = min(gap, a[2] - b[2])
    return final, gap, big


def _ctc_ll(lp, labels, blank):
    """log p(labels | x) by the alpha recursion in float64; lp [V, T] log-probabilities."""
    T = lp.shape[1]
    ext = [blank]
    for c in labels:
        ext += [c, blank]
    if T == 0:
        return 0.0 if not labels else NEG
    alpha = np.full(len(ext), NEG)
    alpha[0] = lp[blank, 0]
    if len(ext) > 1:
        alpha[1] = lp[ext[1], 0]
    for t in range(1, T):
        new = np.full(len(ext), NEG)
        for s in range(len(ext)):
            a = alpha[s]
            if s >= 1:
                a = _ladd(a, alpha[s - 1])
            if s >= 2 and ext[s] != blank and ext[s] != ext[s - 2]:
                a = _ladd(a, alpha[s - 2])
            new[s] = a + lp[ext[s], t] if a != NEG else NEG
        alpha = new
    return _ladd(alpha[-1], alpha[-2] if len(ext) > 1 else NEG)


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------------------
def _inventory(v, blank, n_letters, seed):
    """A piece vocabulary of v classes: the blank at `blank`, <unk>, the bare word start, every letter with and without the word start, and pieces
    of two or three letters, every other one starting a word."""
    rng = np.random.Generator(np.random.PCG64(seed))
    letters = [chr(0x61 + i) for i in range(n_letters)]
    toks = [UNK, WS] + [WS + ch for ch in letters] + letters
    while len(toks) < v - 1:
        body = "".join(letters[int(i)] for i in rng.integers(0, min(n_letters, 4), int(rng.integers(2, 4))))
        tok = (WS if len(toks) % 2 else "") + body
        if tok not in toks:
            toks.append(tok)
    return toks[:blank] + ["<blank>"] + toks[blank:], letters


def _random_fixture(seed, letters, order, n_lex, with_bos=True, with_eos=True, with_unk=True, per_order=150):
    """A random lexicon and word LM: `n_lex` spellings of 1 to 4 letters, mostly over the first four letters and never beginning with the last one
    (a word that begins so is outside the lexicon at its first letter); the LM knows about three quarters of them and three words that the
    lexicon lacks; four hot words -- two that the LM knows, one of the lexicon that it does not, one new to both.  Returns the dictionary over
    word strings, the lexicon list, the hot words."""
    rng = np.random.Generator(np.random.PCG64(seed))
    def spelling():
        n = int(rng.choice([1, 2, 2, 3, 3, 3, 4]))
        return "".join(letters[int(rng.integers(0, 4)) if rng.random() < 0.9 or j == 0 else int(rng.integers(0, len(letters)))] for j in range(n))
    lexicon = []
    while len(lexicon) < n_lex:
        w = spelling()
        if w not in lexicon:
            lexicon.append(w)
    extra = []
    while len(extra) < 4:
        w = spelling()
        if w not in lexicon and w not in extra:
            extra.append(w)
    known = [w for w in lexicon if rng.random() < 0.75]
    unknown = [w for w in lexicon if w not in known]
    lm_words = known + extra[:3]
    hot = sorted(known, key=len)[:2] + sorted(unknown, key=len)[:1] + extra[3:]                  # short ones: the search meets them
    val = lambda n, last: (float(rng.uniform(-3.0, -0.1)), float(rng.uniform(-1.0, 0.0)) if n < order and last != EOS else 0.0)
    grams = {}
    for w in lm_words:
        if rng.random() < 0.9:
            grams[(w,)] = val(1, w)
    for n in range(2, order + 1):
        for _ in range(per_order):
            g = tuple(lm_words[int(rng.integers(len(lm_words)))] for _ in range(n))
            grams[g] = val(n, g[-1])
        for g in [g for g in list(grams) if len(g) == n - 1 and g[0] not in (BOS, EOS) and g[-1] != EOS]:
            if with_bos and rng.random() < 0.3:
                grams[(BOS,) + g] = val(n, g[-1])
            if with_eos and rng.random() < 0.3:
                grams[g + (EOS,)] = val(n, EOS)
    if with_bos:
        grams[(BOS,)] = (-99.0, float(rng.uniform(-1.0, 0.0)))
    if with_eos:
        grams[(EOS,)] = val(1, EOS)
    if with_unk:
        grams[(UNK,)] = val(1, EOS)
    return grams, lexicon, hot


def _package_lm(itos, grams, lexicon, hot, order, blank):
    from thunder_speech_amd.ctc_lm import PieceWordNGramLM
    return PieceWordNGramLM(order, grams, itos, blank, WS, lexicon, hot, None, FLOOR)


# ---- the launch ----------------------------------------------------------------------------------------------------------------------------------
def _launch(logits, n_frames, blank, width, cap, n_best, lm, setting, eos, lengths=None, graph=False):
    """logits: CPU f32 [B, V, pitch]; lm: the package's PieceWordNGramLM; setting: (alpha, beta, oov_score, hotword_weight, boosts).  The workspace
    is pre-filled with 0xFF bytes and the outputs with garbage.  Returns numpy (tokens, frames, lengths, scores, lm_scores, counts)."""
    import ctypes
    from thunder_speech_amd import _lib
    L = _lib.lib()
    b, v, pitch = logits.shape
    lg = logits.cuda()
    il = None if lengths is None else torch.tensor(lengths, dtype=torch.int32).cuda()
    w = lm.weights(*setting)
    assert w.struct.delimiter == -1
    nbytes = L.ts_ctc_beam_piece_lm_workspace_bytes(b, n_frames, width, cap)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    i32 = lambda *s: torch.full(s, -7, dtype=torch.int32, device="cuda")
    f32 = lambda *s: torch.full(s, 7.0, dtype=torch.float32, device="cuda")
    out = [i32(b, n_best, n_frames), i32(b, n_best, n_frames), i32(b, n_best), f32(b, n_best), f32(b, n_best), i32(b)]

    def call():
        st = L.ts_ctc_beam_piece_lm_search(lg.data_ptr(), b, v, n_frames, pitch, None if il is None else il.data_ptr(), blank, width, cap, n_best,
                                           int(eos), ctypes.byref(w.lm.struct), ctypes.byref(w.struct), ctypes.byref(w.pieces),
                                           *[o.data_ptr() for o in out], ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert st == 0, st

    if not graph:
        call()
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in out]
    call()
    torch.cuda.synchronize()
    eager = [o.cpu().numpy().copy() for o in out]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            call()

    def replay():
        for o in out:
            o.fill_(-9)
        ws.fill_(0xFF)
        g.replay()
        torch.cuda.synchronize()
        return [o.cpu().numpy().copy() for o in out]
    replay.keep = (lg, il, w)                                                 # what the graph reads stays allocated as long as the graph is replayed
    return eager, replay


def _launch_plain(logits, n_frames, blank, width, cap, n_best, lengths=None):
    """ts_ctc_beam_search on the same tensors: numpy (tokens, frames, lengths, scores, counts)."""
    from thunder_speech_amd import _lib
    L = _lib.lib()
    b, v, pitch = logits.shape
    lg = logits.cuda()
    il = None if lengths is None else torch.tensor(lengths, dtype=torch.int32).cuda()
    ws = torch.empty(L.ts_ctc_beam_workspace_bytes(b, n_frames, width, cap), dtype=torch.uint8, device="cuda")
    out = [torch.full((b, n_best, n_frames), -7, dtype=torch.int32, device="cuda"), torch.full((b, n_best, n_frames), -7, dtype=torch.int32, device="cuda"),
           torch.full((b, n_best), -7, dtype=torch.int32, device="cuda"), torch.full((b, n_best), 7.0, dtype=torch.float32, device="cuda"),
           torch.full((b,), -7, dtype=torch.int32, device="cuda")]
    st = L.ts_ctc_beam_search(lg.data_ptr(), b, v, n_frames, pitch, None if il is None else il.data_ptr(), blank, width, cap, n_best,
                              *[o.data_ptr() for o in out], ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert st == 0, st
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def _bound(order, T, big):
    return (80 + 16 * order) * (T + 1) * U53 * max(1.0, big)


def _compare(name, got, i, ref, order, T, n_best):
    """Utterance i of `got` against the reference result `ref`: margin, then tokens, frames, lengths, counts equal, scores and lm_scores within
    the tolerance; cells beyond a length or the count are zero, scores beyond the count -inf."""
    tokens, frames, lengths, scores, lm_scores, counts = got
    final, gap, big = ref
    e = _bound(order, T, big)
    print(f"RATIO|beam-piece-lm-margin|{e / gap if gap < math.inf else 0.0:.3e}|{name}[{i}] E / smallest decision gap (E {e:.3e}, gap {gap:.3e})")
    assert gap > e, f"{name}[{i}]: the fixture no longer meets the margin condition ({gap:.3e} <= {e:.3e}); pick another seed"
    want = final[:n_best]
    assert int(counts[i]) == len(want), f"{name}[{i}]: {counts[i]} hypotheses, reference {len(want)}"
    worst = 0.0
    for n in range(n_best):
        if n >= len(want):
            assert lengths[i, n] == 0 and scores[i, n] == NEG and lm_scores[i, n] == 0 and not tokens[i, n].any() and not frames[i, n].any()
            continue
        pre, fr, key, lm10 = want[n]
        assert int(lengths[i, n]) == len(pre), f"{name}[{i}] rank {n}: length {lengths[i, n]}, reference {len(pre)}"
        assert tokens[i, n, : len(pre)].tolist() == list(pre), f"{name}[{i}] rank {n}: tokens"
        assert frames[i, n, : len(pre)].tolist() == list(fr), f"{name}[{i}] rank {n}: frames"
        assert not tokens[i, n, len(pre):].any() and not frames[i, n, len(pre):].any()
        worst = max(worst, abs(float(scores[i, n]) - key) / _tol(key), abs(float(lm_scores[i, n]) - lm10) / _tol(lm10))
        assert abs(float(scores[i, n]) - key) <= _tol(key), f"{name}[{i}] rank {n}: score {scores[i, n]!r}, reference {key!r}"
        assert abs(float(lm_scores[i, n]) - lm10) <= _tol(lm10), f"{name}[{i}] rank {n}: lm_score {lm_scores[i, n]!r}, reference {lm10!r}"
    print(f"RATIO|beam-piece-lm-score|{worst:.3e}|{name}[{i}] (T {T}, {len(want)} hypotheses)")


def _randn(seed, shape, scale=3.0):
    return (scale * np.random.Generator(np.random.PCG64(seed)).standard_normal(shape)).astype(np.float32)


def _kinds(k, pre):
    """What a prefix shows of the child rule, read off its text."""
    kinds, words = set(), [w for w in k.text(pre).replace(WS, " ").split(" ") if w]
    kinds |= {"in" if w in k.lexicon else "out" for w in words}
    kinds |= {"hot"} if any(w in k.hot for w in words) else set()
    kinds |= {"pending"} if k.pending(pre) else set()
    for j, c in enumerate(pre):
        tok, cur = k.itos[c], k.pending(pre[:j])
        kinds |= {"bare"} if tok == WS else set()
        kinds |= {"no-spelling"} if k.piece(c) == "?" else set()
        if tok.startswith(WS) and len(tok) > 1 and cur and tok[1:] not in k.begins:
            kinds.add("ends-a-word-and-leaves")                              # one child: the word's end and the next word's OOV factor
        body = tok[1:] if tok.startswith(WS) else tok
        start = "" if tok.startswith(WS) else cur
        if k.piece(c) != "?" and len(body) > 1 and start in k.begins and start + body[:1] in k.begins and start + body not in k.begins:
            kinds.add("leaves-mid-piece")
    return kinds


def _script(k, letters):
    """Classes that a clip "says", so that the beams meet every branch of the child rule: a hot word letter by letter, a bare word start, a lexicon
    word in continuation pieces, a piece of several letters that leaves the lexicon after its first, a word-start piece that ends that word and is
    outside the lexicon at once (no word begins with the last letter), a class without a spelling, and a word that stays pending."""
    cls = k.itos.index
    words = sorted(k.lexicon, key=lambda w: (len(w), w))
    hot = sorted((w for w in k.hot if w in k.lexicon), key=lambda w: (len(w), w))[0]
    inw = [w for w in words if w != hot and len(w) >= 2][0]
    seq = [cls(WS + hot[0])] + [cls(ch) for ch in hot[1:]] + [cls(WS)] + [cls(ch) for ch in inw]
    mid = None
    for tok in k.itos:
        body = tok[1:] if tok.startswith(WS) else tok
        if tok in ("<blank>", UNK) or len(body) < 2 or mid:
            continue
        for first in ([""] if tok.startswith(WS) else letters[:4]):
            if first + body[0] in k.begins and first + body not in k.begins and not mid:
                mid = ([cls(WS + first)] if first else []) + [cls(tok)]
    assert mid, "no piece of this inventory leaves this lexicon after its first letter"
    return seq + mid + [cls(WS + letters[-1]), cls(UNK), cls(WS + inw[0])] + [cls(ch) for ch in inw[1:]]


# ---- 1. random cases against the reference -------------------------------------------------------------------------------------------------------
ALPHA, BETA, OOV, HOT_W = 0.7, 0.6, -2.5, 1.5            # the setting of the random cases; one hot word has a boost of its own (3.0)
RANDOM = {  # name: V, letters, T, beam_width, token_cap, blank, lengths (one per clip), n_lex, (with <s>, </s>, <unk>), seed
    "v16-t50-w8-c4": (16, 5, 50, 8, 4, 0, [50], 40, (True, True, True), 0),
    "v16-t50-w16-c7": (16, 5, 50, 16, 7, 0, [50], 40, (True, True, False), 1),
    "v70-t40-w16-c8": (70, 8, 40, 16, 8, 69, [40], 60, (False, True, True), 2),          # n_classes > BEAM_ROW: the stay candidates read the logits
    "b4-v16-t30-w8-c4-lengths": (16, 5, 30, 8, 4, 7, [30, 0, 17, 1], 40, (True, True, True), 3),   # a batch with lengths, one clip empty
    "v40-t24-w64-c15": (40, 6, 24, 64, 15, 11, [24], 50, (True, True, True), 4),         # 1024 candidates: the rank count in chunks of 64 keys
}
ORDER = 3
EVERY_KIND = {"in", "out", "hot", "pending", "bare", "no-spelling", "ends-a-word-and-leaves", "leaves-mid-piece"}


@functools.lru_cache(maxsize=None)
def _random_case(name):
    """The logits [B, V, pitch] (pitch > T, NaN in every cell beyond a length), the fixture and per (utterance, eos) the reference: computed once."""
    v, n_letters, T, width, cap, blank, lengths, n_lex, (bos, eos, unk), seed = RANDOM[name]
    itos, letters = _inventory(v, blank, n_letters, 900 + seed)
    grams, lexicon, hot = _random_fixture(700 + seed, letters, ORDER, n_lex, bos, eos, unk)
    boosts = {w: HOT_W for w in hot}
    boosts[hot[1]] = 3.0
    k = _Strings(itos, blank, grams, ORDER, list(lexicon) + list(hot), boosts, ALPHA, BETA, OOV)
    script = _script(k, letters)
    x = np.full((len(lengths), v, T + 9), np.nan, np.float32)
    for i, n in enumerate(lengths):
        x[i, :, :n] = _randn(60 + 10 * seed + i, (v, n), 2.0)
        x[i, blank, 1:n:2] += 9.0                                           # a piece every other frame: the script, against the noise
        for j, c in enumerate(script[: (n + 1) // 2]):
            x[i, c, 2 * j] += 18.0
    refs = {(i, e): _search_piece(x[i, :, :n], width, cap, k, e) for i, n in enumerate(lengths) for e in (False, True)}
    return x, (itos, grams, lexicon, hot, {hot[1]: 3.0}), k, refs


@pytest.mark.gpu
@pytest.mark.parametrize("score_eos", [True, False], ids=["eos", "no-eos"])
@pytest.mark.parametrize("name", list(RANDOM))
def test_equals_the_reference_where_the_margin_condition_holds(name, score_eos):
    v, _, T, width, cap, blank, lengths, _, _, _ = RANDOM[name]
    x, (itos, grams, lexicon, hot, own), k, refs = _random_case(name)
    lm = _package_lm(itos, grams, lexicon, hot, ORDER, blank)
    assert sorted(lm.words) == sorted(k.lexicon) and lm.unspellable_classes == [itos.index(UNK)] and lm.dropped == 0
    n_best = min(width, 8)
    got = _launch(torch.from_numpy(x), T, blank, width, cap, n_best, lm, (ALPHA, BETA, OOV, HOT_W, own), score_eos, lengths)
    for i, n in enumerate(lengths):
        _compare(name, got, i, refs[(i, score_eos)], ORDER, n, n_best)
    # the final beams meet every branch of the child rule
    kinds = set()
    for i in range(len(lengths)):
        for pre, _, _, _ in refs[(i, score_eos)][0]:
            kinds |= _kinds(k, pre)
    assert kinds == EVERY_KIND, EVERY_KIND - kinds


# ---- 2. exhaustive: scores are CTC likelihood + LM + word bonus + OOV scores + boosts -----------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("score_eos", [True, False], ids=["eos", "no-eos"])
def test_every_score_is_the_ctc_likelihood_plus_the_word_lm_plus_the_word_terms(score_eos):
    """3 non-blank classes ("▁a", "t", "▁"), T = 3, beam 64: the 25 feasible label strings (1 + 3 + 9 + the 12 of three labels without a repeat, which
    would need a blank it has no frame for) never fill the beam, so nothing is pruned and the score of every hypothesis is its full CTC
    log-likelihood + alpha ln 10 LM(words, the pending word included) + beta (words) + oov_score (OOV words) + the boosts of its hot words
    (+ </s>).  "▁a t" and "▁a ▁ t" are two hypotheses whose words differ; "▁a t" and "▁ ▁a t" -- and "t" and "▁ t" -- are segmentations that spell the
    same words: each is a hypothesis of its own, with the same LM score and its own CTC likelihood."""
    itos, blank, T, width, cap = ["▁a", "<blank>", "t", WS], 1, 3, 64, 3
    alpha, beta, oov, hot_w = 0.8, 0.6, -1.7, 1.1
    grams = {(BOS,): (-99.0, -0.3), (EOS,): (-1.2, 0.0), (UNK,): (-2.0, 0.0), ("a",): (-0.7, -0.2), ("at",): (-1.1, -0.4), ("ta",): (-1.3, -0.1),
             (BOS, "a"): (-0.4, -0.15), ("a", "at"): (-0.6, -0.25), ("at", EOS): (-0.5, 0.0), ("a", "a"): (-0.9, -0.05), (BOS, "a", "at"): (-0.35, 0.0),
             ("a", "a", EOS): (-0.45, 0.0)}
    lexicon, hot = ["a", "at", "ta", "tt"], ["at", "tt"]                     # "tt" is in the lexicon and not in the LM; "t" is outside both
    lm = _package_lm(itos, grams, lexicon, hot, 3, blank)
    k = _Strings(itos, blank, grams, 3, lexicon, {w: hot_w for w in hot}, alpha, beta, oov)
    x = _randn(177, (4, T), 1.5)
    ref = _search_piece(x, width, cap, k, score_eos)
    assert len(ref[0]) == 25
    got = _launch(torch.from_numpy(x)[None].contiguous(), T, blank, width, cap, 64, lm, (alpha, beta, oov, hot_w, None), score_eos)
    _compare("exhaustive", got, 0, ref, 3, T, 64)
    tokens, frames, lengths, scores, lm_scores, counts = got
    assert counts[0] == 25
    lp = _log_softmax64(x)
    worst, by_words = 0.0, {}
    for n in range(25):
        s = tokens[0, n, : lengths[0, n]].tolist()
        words = [w for w in "".join(itos[c] for c in s).replace(WS, " ").split(" ") if w]
        hist, lm10, extra = k.start, 0.0, 0.0
        for w in words:
            key = w if w in k.lexicon and w in k.known else UNKW
            p, fell = _textbook(k.grams, 3, hist, key)
            lm10, hist = lm10 + p, (() if fell else hist + (key,))
            extra += beta + (k.hot.get(w, 0.0) if w in k.lexicon else oov)
        if score_eos:
            lm10 += _textbook(k.grams, 3, hist, EOS)[0]
        want = _ctc_ll(lp, s, blank) + alpha * LN10 * lm10 + extra
        worst = max(worst, abs(float(scores[0, n]) - want) / _tol(want))
        assert abs(float(scores[0, n]) - want) <= _tol(want), f"rank {n} {s}: {scores[0, n]!r} against {want!r}"
        assert abs(float(lm_scores[0, n]) - lm10) <= _tol(lm10)
        by_words.setdefault(tuple(words), []).append(tuple(s))
    # prefixes are sequences of classes: several segmentations spell the same words and stay apart, and one bare word start splits "at" in two
    assert sorted(by_words[("a",)]) == [(0,), (0, 3), (3, 0), (3, 0, 3)] and sorted(by_words[("at",)]) == [(0, 2), (0, 2, 3), (3, 0, 2)]
    assert sorted(by_words[("t",)]) == [(2,), (2, 3), (3, 2), (3, 2, 3)] and by_words[("a", "t")] == [(0, 3, 2)] and by_words[("tt",)] == [(2, 2)]
    print(f"RATIO|beam-piece-lm-exhaustive-score|{worst:.3e}|T {T}, 25 strings")


# ---- 3. all weights zero is the search without an LM ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["v16-t50-w16-c7", "v70-t40-w16-c8", "b4-v16-t30-w8-c4-lengths", "v40-t24-w64-c15"])
def test_with_every_weight_zero_it_agrees_with_the_plain_search(name):
    v, _, T, width, cap, blank, lengths, _, _, _ = RANDOM[name]
    x, (itos, grams, lexicon, hot, _), _, _ = _random_case(name)
    lm = _package_lm(itos, grams, lexicon, hot, ORDER, blank)
    n_best = min(width, 8)
    free = _Strings(itos, blank, {}, 1, set(), {}, 0.0, 0.0, 0.0)
    for i, n in enumerate(lengths):                                           # the plain search's own margin, on the weight-free reference
        _, gap, big = _search_piece(x[i, :, :n], width, cap, free, False)
        assert gap > _bound(ORDER, n, big)
    plain = _launch_plain(torch.from_numpy(x), T, blank, width, cap, n_best, lengths)
    for eos in (True, False):
        tokens, frames, out_len, scores, lm_scores, counts = _launch(torch.from_numpy(x), T, blank, width, cap, n_best, lm, (0.0, 0.0, 0.0, 0.0, None),
                                                                     eos, lengths)
        assert tokens.tobytes() == plain[0].tobytes() and frames.tobytes() == plain[1].tobytes()
        assert out_len.tobytes() == plain[2].tobytes() and counts.tobytes() == plain[4].tobytes()
        for a, p in zip(scores.reshape(-1), plain[3].reshape(-1)):
            assert a == p or abs(float(a) - float(p)) <= _tol(float(p))      # (equal: -inf beyond a count)
        for i in range(len(lengths)):                                      # the LM is still reported
            for n in range(int(counts[i])):
                want = lm.score(tokens[i, n, : out_len[i, n]].tolist(), eos)
                assert abs(float(lm_scores[i, n]) - want) <= _tol(want)


# ---- 4. behaviour: the LM, a hot word and the OOV score change the answer ------------------------------------------------------------------------
TINY = ["<blank>", "<unk>", "▁", "▁a", "▁c", "▁ca", "▁cat", "▁s", "a", "c", "e", "o", "s", "t", "at"]


def _c_vowel_t(first, second, third=None):
    """Seven frames that say ▁c, blank, a vowel, blank, t, blank, blank; the vowel frame prefers `first` to `second` (to `third`) by half a logit."""
    x = -4.0 + 0.05 * _randn(5, (len(TINY), 7), 1.0)                          # (the noise keeps the also-rans from tying)
    for t, c in enumerate([TINY.index("▁c"), 0, None, 0, TINY.index("t"), 0, 0]):
        if c is not None:
            x[c, t] = 6.0
    x[TINY.index(first), 2], x[TINY.index(second), 2] = 5.5, 5.0
    if third:
        x[TINY.index(third), 2] = 4.5
    return x


def _texts(got):
    tokens, _, lengths, _, _, counts = got
    return [" ".join(TINY[c] for c in tokens[0, n, : lengths[0, n]]) for n in range(int(counts[0]))]


@pytest.mark.gpu
def test_an_lm_that_prefers_cat_turns_cot_into_cat_and_a_hot_word_turns_it_back():
    from thunder_speech_amd.ctc_lm import PieceWordNGramLM
    x = _c_vowel_t("o", "a")
    lg = torch.from_numpy(x)[None].contiguous()
    plain = _launch_plain(lg, 7, 0, 8, 4, 2)
    assert [TINY[c] for c in plain[0][0, 0, : plain[2][0, 0]]] == ["▁c", "o", "t"]
    lm = PieceWordNGramLM.from_arpa(ARPA, TINY, 0, hotwords=["cot"])
    fused = _launch(lg, 7, 0, 8, 4, 2, lm, (1.0, 0.0, -10.0, 0.0, None), True)
    assert _texts(fused) == ["▁c a t", "▁c o t"]
    # <s> cat </s>: the bigram, then back-off(<s> cat) and the bigram; <s> cot </s>: both back off to the unigrams
    assert abs(float(fused[4][0, 0]) - (-0.7 - 0.1 - 0.8)) <= _tol(1.6) and abs(float(fused[4][0, 1]) - (-0.4 - 1.6 - 0.1 - 1.1)) <= _tol(3.2)
    assert _texts(_launch(lg, 7, 0, 8, 4, 2, lm, (0.0, 0.0, -10.0, 0.0, None), True))[0] == "▁c o t"
    # the LM alone loses "cot" by 1.7 ln 10 - 0.5 = 3.4; a boost of 5 wins it back, and lm_scores do not see the boost
    hot = _launch(lg, 7, 0, 8, 4, 2, lm, (1.0, 0.0, -10.0, 5.0, None), True)
    assert _texts(hot) == ["▁c o t", "▁c a t"] and abs(float(hot[4][0, 0]) - (-0.4 - 1.6 - 0.1 - 1.1)) <= _tol(3.2)
    assert abs(float(hot[3][0, 0]) - (float(fused[3][0, 1]) + 5.0)) <= 2 * _tol(float(hot[3][0, 0]))
    assert _texts(_launch(lg, 7, 0, 8, 4, 2, lm, (1.0, 0.0, -10.0, 0.0, {"cot": 5.0}), True)) == ["▁c o t", "▁c a t"]


@pytest.mark.gpu
def test_a_large_negative_oov_score_keeps_an_out_of_lexicon_spelling_out_of_the_1_best():
    from thunder_speech_amd.ctc_lm import PieceWordNGramLM
    x = _c_vowel_t("e", "a", "o")                                             # the acoustic model hears "cet", which is no word
    lg = torch.from_numpy(x)[None].contiguous()
    lm = PieceWordNGramLM.from_arpa(ARPA, TINY, 0)
    assert _texts(_launch(lg, 7, 0, 8, 4, 3, lm, (0.0, 0.0, 0.0, 0.0, None), True))[0] == "▁c e t"
    kept_out = _launch(lg, 7, 0, 8, 4, 3, lm, (0.0, 0.0, -20.0, 0.0, None), True)
    assert _texts(kept_out)[:2] == ["▁c a t", "▁c o t"] and "▁c e t" not in _texts(kept_out)[:2]


# ---- 5. bookkeeping ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_captured_call_replays_the_eager_bits_and_a_new_setting_leaves_the_old_graph_alone():
    """PieceWordNGramLM.weights gives a NEW cached setting for new boosts -- new word_factor / oov_factor tensors, nothing written at the old
    addresses -- so the graph captured under the old setting replays the old setting's bits."""
    name = "b4-v16-t30-w8-c4-lengths"
    v, _, T, width, cap, blank, lengths, _, _, _ = RANDOM[name]
    x, (itos, grams, lexicon, hot, own), _, _ = _random_case(name)
    lm = _package_lm(itos, grams, lexicon, hot, ORDER, blank)
    old = (ALPHA, BETA, OOV, HOT_W, own)
    eager, replay = _launch(torch.from_numpy(x), T, blank, width, cap, 4, lm, old, True, lengths, graph=True)
    first = replay()
    again = _launch(torch.from_numpy(x), T, blank, width, cap, 4, lm, old, True, lengths)
    for a, r, c in zip(eager, first, again):
        assert a.tobytes() == r.tobytes() == c.tobytes()
    w_old = lm.weights(*old)
    new = (ALPHA, BETA, OOV, HOT_W, {hot[0]: 9.0, hot[1]: -4.0})
    w_new = lm.weights(*new)
    assert w_new is not w_old and lm.weights(*old) is w_old and lm.weights(*new) is w_new
    assert w_new.tensors["word_factor"].data_ptr() != w_old.tensors["word_factor"].data_ptr()
    assert w_new.tensors["oov_factor"].data_ptr() != w_old.tensors["oov_factor"].data_ptr()
    for fixed in ("edge_begin", "piece_begin", "piece_letter", "piece_kind"):                       # the trie and the pieces do not depend on the setting
        assert w_new.tensors[fixed].data_ptr() == w_old.tensors[fixed].data_ptr()
    other = _launch(torch.from_numpy(x), T, blank, width, cap, 4, lm, new, True, lengths)
    assert other[3].tobytes() != eager[3].tobytes()                           # the new boosts change scores
    for a, r in zip(eager, replay()):
        assert a.tobytes() == r.tobytes()                                     # the replay under the old setting is unchanged


@pytest.mark.gpu
def test_cells_beyond_lengths_and_counts_and_the_empty_clip():
    """T = 0 gives the empty hypothesis (no pending word; with </s> its score is alpha ln 10 log10 P(</s> | <s>)); a one-frame clip has as many
    hypotheses as it has candidates + 1, so ranks beyond stay empty: zero tokens, frames, lengths and lm_scores, -inf scores.  _launch pre-fills
    the workspace with 0xFF bytes and the outputs with garbage."""
    name = "b4-v16-t30-w8-c4-lengths"
    v, _, T, width, cap, blank, lengths, _, _, _ = RANDOM[name]
    x, (itos, grams, lexicon, hot, own), k, refs = _random_case(name)
    lm = _package_lm(itos, grams, lexicon, hot, ORDER, blank)
    setting = (ALPHA, BETA, OOV, HOT_W, own)
    n_best = 8
    for eos in (True, False):
        got = _launch(torch.from_numpy(x), T, blank, width, cap, n_best, lm, setting, eos, lengths)
        tokens, frames, out_len, scores, lm_scores, counts = got
        assert counts.tolist() == [n_best, 1, n_best, cap + 1]
        want10 = _textbook(k.grams, ORDER, k.start, EOS)[0] if eos else 0.0
        assert out_len[1, 0] == 0 and abs(float(scores[1, 0]) - ALPHA * LN10 * want10) <= _tol(ALPHA * LN10 * want10)
        assert abs(float(lm_scores[1, 0]) - want10) <= _tol(want10)
        assert (scores[1, 1:] == NEG).all() and (scores[3, cap + 1:] == NEG).all() and not lm_scores[1, 1:].any() and not lm_scores[3, cap + 1:].any()
        assert not out_len[1].any() and not out_len[3, cap + 1:].any() and not tokens[1].any() and not frames[1].any() and not tokens[3, cap + 1:].any()
        for i, n in enumerate(lengths):
            assert not tokens[i, :, n:].any() and not frames[i, :, n:].any()
    clamped = _launch(torch.from_numpy(x), T, blank, width, cap, n_best, lm, setting, True, [T + 50, -3, 17, 1])
    for a, c in zip(_launch(torch.from_numpy(x), T, blank, width, cap, n_best, lm, setting, True, lengths), clamped):
        assert a.tobytes() == c.tobytes()                                      # lengths outside [0, n_frames] are clamped


# ---- 6. through the module -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_predict_beam_and_predict_nbest_with_a_piece_lm_through_the_module():
    """The random tiny Citrinet of citrinet/compatibility.py with the test's pieces as its vocabulary (the blank comes last there): predict_beam and
    predict_nbest with the LM are beam_search_piece_lm on the module's logits."""
    from thunder_speech_amd.citrinet.compatibility import build_synthetic_citrinet
    from thunder_speech_amd.ctc_lm import PieceWordNGramLM, beam_search_piece_lm
    from thunder_speech_amd.text_processing.transform import BatchTextTransformer
    torch.manual_seed(3)
    module = build_synthetic_citrinet(filters=[64, 128], kernel_sizes=[5, 7], strides=[2, 1], n_tokens=len(TINY) - 1)
    module.text_transform = BatchTextTransformer(tokens=TINY[1:])
    module = module.cuda().eval()
    vocab = module.text_transform.vocab
    assert vocab.itos == TINY[1:] + ["<blank>"] and vocab.blank_idx == 14
    lm = PieceWordNGramLM.from_arpa(ARPA, vocab.itos, vocab.blank_idx, hotwords=["cot"])
    rng = np.random.Generator(np.random.PCG64(7))
    x = torch.from_numpy((0.1 * rng.standard_normal((2, 16000))).astype(np.float32)).cuda()
    kw = dict(alpha=0.5, beta=1.0, oov_score=-1.0, hotword_weight=2.0, boosts={"cot": 3.0})
    logits = module._eval_logits(x, None)[0]
    assert logits.shape[:2] == (2, 15)
    direct = beam_search_piece_lm(logits, lm, kw["alpha"], kw["beta"], None, 14, 8, 4, 3, True, kw["oov_score"], kw["hotword_weight"], kw["boosts"])
    tokens, out_len, scores, lm_scores, counts = (t.cpu().numpy() for t in (direct.tokens, direct.lengths, direct.scores, direct.lm_scores, direct.counts))
    fused = module.predict_nbest(x, 3, beam_width=8, token_cap=4, lm=lm, **kw)
    assert len(fused) == 2
    for i, clip in enumerate(fused):
        assert len(clip) == int(counts[i]) >= 1
        for n, h in enumerate(clip):
            ids = tokens[i, n, : out_len[i, n]].tolist()
            assert [t.token for t in h.tokens] == [vocab.itos[c] for c in ids] and h.text == module.text_transform._ids_to_text(ids)
            assert h.score == float(scores[i, n]) and h.lm_score == float(lm_scores[i, n])
            want = lm.score(ids, eos=True)
            assert abs(h.lm_score - want) <= _tol(want)
    assert module.predict_beam(x, beam_width=8, token_cap=4, lm=lm, **kw) == [clip[0].text for clip in fused]
    zero = dict(alpha=0.0, beta=0.0, oov_score=0.0, hotword_weight=0.0)
    assert module.predict_beam(x, beam_width=8, token_cap=4, lm=lm, **zero) == module.predict_beam(x, beam_width=8, token_cap=4)
    other = PieceWordNGramLM.from_arpa(ARPA, vocab.itos[:5] + ["▁co"] + vocab.itos[6:], vocab.blank_idx)
    with pytest.raises(ValueError, match="class 5 is '▁co' there and '▁cat' in this module"):
        module.predict_beam(x, lm=other)
    with pytest.raises(ValueError, match="class 5 is '▁co' there and '▁cat' in this module"):
        module.predict_nbest(x, 2, lm=other)
