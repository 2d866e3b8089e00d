"""CTC prefix beam search with a word-level n-gram LM, a lexicon and hot words on the GPU (include_open/thunder_speech_amd/ctc_beam_word_lm.h,
csrc/ctc_beam_word_lm.hip) through the raw C ABI and through the module.

The reference is `_search_word` below: the header's algorithm restated in float64 in the LOG domain, in the style of `_search_lm` of
tests/test_gpu_ctc_beam_lm.py, with prefixes as tuples (no hashes, no trie, no automaton).  The lexicon is a plain set of spellings; the lexicon
state of a prefix is read off the letters after its last delimiter ("is it a spelling, is it the beginning of one"), and the LM score of a
word is read from the n-gram DICTIONARY by the textbook back-off (`_textbook`), the context being the words so far (emptied by a word that took
the floor).  Nothing of the package takes part in it.  Independent of that restatement, the exhaustive case compares every score with CTC
log-likelihood (plain float64 alpha recursion) + alpha ln 10 LM(words) + beta (words) + oov_score (OOV words) + boosts (+ </s>), the words
found by splitting the labels at the delimiter.

Tolerance of a score and of an lm_score: 2^-23 max(1, |value|) -- the one f32 rounding (2^-24 relative) plus float64 noise.

The margin condition (asserted by every test that demands equal tokens) is that of tests/test_gpu_ctc_beam_lm.py, whose count per frame and side
is fewer than 32 + 4 N + 4 ulp (N the LM's order), with the two extra products a child can meet added: on the device the hot-word factor and the
OOV factor, each one f64 product by a factor that carries up to 2 ulp of its own (one exponential on the host) -- 6 ulp relative; in the
reference the two matching sums (the boost, the OOV score) -- 2 roundings, each an absolute error of an ulp of the magnitude of its partial sum,
at most max(M, L), M the largest |log key| and L the largest |alpha ln 10 log10 p + beta + boost + oov_score| of a child.  Fewer than
32 + 4 N + 4 + 6 <= 40 + 8 N ulp per frame on either side.  The pending word after the last frame is one more such step (and the one </s>
product is covered by the slack of the first term), so the errors add up linearly over T + 1 steps: two log keys closer than
E = (80 + 16 N) (T + 1) 2^-53 max(1, M, L) may fall either way, and the tests require the smallest gap (last kept key against first dropped key
over all frames, and neighbouring keys of the final beam after the pending words and </s>) to exceed E.  The fixtures' margins were measured on the
CPU before the seeds were fixed (>= 2e-4 against E <= 6e-11); the assertion stays in every test.

Ratios error / bound are printed as `RATIO|kind|ratio|case`."""
import functools
import itertools
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
BOS, EOS, UNK = -1, -2, -3                                                   # ids of <s>, </s>, <unk> inside the n-gram dictionaries
UNKW = "a word the LM does not know"                                         # what such a word is looked up as: in no n-gram
FLOOR = -10.0                                                                # log10 p of a word without a unigram in an LM without <unk>


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


class _Words:
    """What the reference knows: the n-gram dictionary over words (a word is the tuple of its classes), the lexicon as a set of such tuples, the
    boost of each hot word, and the four weights."""

    def __init__(self, grams, order, lexicon, hot, delim, alpha, beta, oov_score):
        self.grams, self.order, self.lexicon, self.hot, self.delim = grams, order, set(lexicon), dict(hot), delim
        self.alpha, self.beta, self.oov_score = alpha, beta, oov_score
        self.begins = {w[:k] for w in self.lexicon for k in range(len(w) + 1)} | {()}           # what a spelling of the lexicon can begin with
        self.known = {w for g in grams for w in g if isinstance(w, tuple)}                      # the LM's words
        self.has_eos = any(g[-1] == EOS for g in grams)
        self.start = (BOS,) if any(g[0] == BOS for g in grams) else ()

    def pending(self, pre):
        """The letters after the last delimiter of a prefix."""
        k = len(pre)
        while k > 0 and pre[k - 1] != self.delim:
            k -= 1
        return tuple(pre[k:])

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
        cur = self.pending(pre)
        if c != self.delim:
            return (self.oov_score if cur in self.begins and cur + (c,) not in self.begins else 0.0), 0.0, hist
        if not cur:
            return 0.0, 0.0, hist
        return self.end_word(cur, hist)


def _search_word(x, blank, width, cap, k, eos):
    """x [V, T] f32, k a _Words -> (final beam [(prefix, frames, log key, log10 LM score)], smallest decision gap, largest magnitude): the header,
    word by word."""
    V, T = x.shape
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
def _itos(v, blank, delim):
    """Single-character classes: the blank, the delimiter " " and letters."""
    letters = iter(chr(0x61 + i) if i < 26 else chr(0x100 + i) for i in range(v))
    return ["<blank>" if c == blank else " " if c == delim else next(letters) for c in range(v)]


def _random_fixture(seed, v, blank, delim, common, order, n_lex, with_bos=True, with_eos=True, with_unk=True, per_order=150):
    """A random lexicon and word LM over the classes `common` (the letters the logits prefer) and, rarely, the others: `n_lex` spellings of 1 to 4
    letters; the LM knows about three quarters of them and three words that the lexicon lacks; four hot words -- two that the LM knows, one of
    the lexicon that it does not, one new to both.  Returns the dictionary over WORD STRINGS (for the package), the lexicon list, the hot words."""
    rng = np.random.Generator(np.random.PCG64(seed))
    itos = _itos(v, blank, delim)
    letters = [c for c in range(v) if c not in (blank, delim)]
    def spelling():
        n = int(rng.choice([1, 2, 2, 3, 3, 3, 4]))
        return "".join(itos[int(rng.choice(common)) if rng.random() < 0.9 else int(rng.choice(letters))] for _ in range(n))
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
    val = lambda n, last: (float(rng.uniform(-3.0, -0.1)), float(rng.uniform(-1.0, 0.0)) if n < order and last != "</s>" else 0.0)
    grams = {}
    for w in lm_words:
        if rng.random() < 0.9:
            grams[(w,)] = val(1, w)
    for n in range(2, order + 1):
        for _ in range(per_order):
            g = tuple(lm_words[int(rng.integers(len(lm_words)))] for _ in range(n))
            grams[g] = val(n, g[-1])
        for g in [g for g in list(grams) if len(g) == n - 1 and g[0] not in ("<s>", "</s>") and g[-1] != "</s>"]:
            if with_bos and rng.random() < 0.3:
                grams[("<s>",) + g] = val(n, g[-1])
            if with_eos and rng.random() < 0.3:
                grams[g + ("</s>",)] = val(n, "</s>")
    if with_bos:
        grams[("<s>",)] = (-99.0, float(rng.uniform(-1.0, 0.0)))
    if with_eos:
        grams[("</s>",)] = val(1, "</s>")
    if with_unk:
        grams[("<unk>",)] = val(1, "</s>")
    return itos, grams, lexicon, hot


def _reference_words(itos, grams, lexicon, hot, boosts, order, delim, alpha, beta, oov_score):
    """The fixture as the reference wants it: words as tuples of classes; `boosts` maps every hot word to its boost."""
    special = {"<s>": BOS, "</s>": EOS, "<unk>": UNK}
    sp = lambda w: tuple(itos.index(ch) for ch in w)
    g = {tuple(special[w] if w in special else sp(w) for w in gram): val for gram, val in grams.items()}
    return _Words(g, order, {sp(w) for w in list(lexicon) + list(hot)}, {sp(w): boosts[w] for w in hot}, delim, alpha, beta, oov_score)


def _package_lm(itos, grams, lexicon, hot, order, blank):
    from thunder_speech_amd.ctc_lm import WordNGramLM
    return WordNGramLM(order, grams, itos, blank, " ", lexicon, hot, None, FLOOR)


# ---- the launch ----------------------------------------------------------------------------------------------------------------------------------
def _launch(logits, n_frames, blank, width, cap, n_best, lm, setting, eos, lengths=None, graph=False):
    """logits: CPU f32 [B, V, pitch]; lm: the package's WordNGramLM; setting: (alpha, beta, oov_score, hotword_weight, boosts).  The workspace is
    pre-filled with 0xFF bytes and the outputs with garbage.  Returns numpy (tokens, frames, lengths, scores, lm_scores, counts)."""
    import ctypes
    from thunder_speech_amd import _lib
    L = _lib.lib()
    b, v, pitch = logits.shape
    lg = logits.cuda()
    il = None if lengths is None else torch.tensor(lengths, dtype=torch.int32).cuda()
    w = lm.weights(*setting)
    nbytes = L.ts_ctc_beam_word_lm_workspace_bytes(b, n_frames, width, cap)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    i32 = lambda *s: torch.full(s, -7, dtype=torch.int32, device="cuda")
    f32 = lambda *s: torch.full(s, 7.0, dtype=torch.float32, device="cuda")
    out = [i32(b, n_best, n_frames), i32(b, n_best, n_frames), i32(b, n_best), f32(b, n_best), f32(b, n_best), i32(b)]

    def call():
        st = L.ts_ctc_beam_word_lm_search(lg.data_ptr(), b, v, n_frames, pitch, None if il is None else il.data_ptr(), blank, width, cap, n_best,
                                          int(eos), ctypes.byref(w.lm.struct), ctypes.byref(w.struct), *[o.data_ptr() for o in out], ws.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream)
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
    print(f"RATIO|beam-word-lm-margin|{e / gap if gap < math.inf else 0.0:.3e}|{name}[{i}] E / smallest decision gap (E {e:.3e}, gap {gap:.3e})")
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
    print(f"RATIO|beam-word-lm-score|{worst:.3e}|{name}[{i}] (T {T}, {len(want)} hypotheses)")


def _randn(seed, shape, scale=3.0):
    return (scale * np.random.Generator(np.random.PCG64(seed)).standard_normal(shape)).astype(np.float32)


# ---- 1. random cases against the reference -------------------------------------------------------------------------------------------------------
ALPHA, BETA, OOV, HOT_W = 0.7, 0.6, -2.5, 1.5            # the setting of the random cases; one hot word has a boost of its own (3.0)
RANDOM = {  # name: V, T, beam_width, token_cap, blank, delimiter, lengths (one per clip), n_lex, (with <s>, </s>, <unk>), seed
    "v8-t50-w8-c4": (8, 50, 8, 4, 0, 1, [50], 40, (True, True, True), 8),
    "v8-t50-w16-c7": (8, 50, 16, 7, 0, 1, [50], 40, (True, True, False), 1),
    "v70-t40-w16-c8": (70, 40, 16, 8, 69, 3, [40], 60, (False, True, True), 2),          # n_classes > BEAM_ROW: the stay candidates read the logits
    "b4-v8-t30-w8-c4-lengths": (8, 30, 8, 4, 7, 2, [30, 0, 17, 1], 40, (True, True, True), 3),   # a batch with lengths, one clip empty
}
ORDER = 3


@functools.lru_cache(maxsize=None)
def _random_case(name):
    """The logits [B, V, pitch] (pitch > T, NaN in every cell beyond a length), the fixture and per (utterance, eos) the reference: computed once."""
    v, T, width, cap, blank, delim, lengths, n_lex, (bos, eos, unk), seed = RANDOM[name]
    letters = [c for c in range(v) if c not in (blank, delim)]
    common = letters[:5]
    itos, grams, lexicon, hot = _random_fixture(700 + seed, v, blank, delim, common, ORDER, n_lex, bos, eos, unk)
    boosts = {w: HOT_W for w in hot}
    boosts[hot[1]] = 3.0
    k = _reference_words(itos, grams, lexicon, hot, boosts, ORDER, delim, ALPHA, BETA, OOV)
    x = np.full((len(lengths), v, T + 9), np.nan, np.float32)
    for i, n in enumerate(lengths):
        x[i, :, :n] = _randn(60 + 10 * seed + i, (v, n))
        x[i, common, :n] += 4.0 if v > 8 else 0.5
        x[i, delim, :n] += 5.0 if v > 8 else 2.0                            # words of a few letters
    refs = {(i, e): _search_word(x[i, :, :n], blank, width, cap, k, e) for i, n in enumerate(lengths) for e in (False, True)}
    return x, (itos, grams, lexicon, hot, {hot[1]: 3.0}), k, refs


@pytest.mark.gpu
@pytest.mark.parametrize("score_eos", [True, False], ids=["eos", "no-eos"])
@pytest.mark.parametrize("name", list(RANDOM))
def test_equals_the_reference_where_the_margin_condition_holds(name, score_eos):
    v, T, width, cap, blank, delim, lengths, _, _, _ = RANDOM[name]
    x, (itos, grams, lexicon, hot, own), k, refs = _random_case(name)
    lm = _package_lm(itos, grams, lexicon, hot, ORDER, blank)
    assert lm.delimiter == delim
    n_best = min(width, 8)
    got = _launch(torch.from_numpy(x), T, blank, width, cap, n_best, lm, (ALPHA, BETA, OOV, HOT_W, own), score_eos, lengths)
    for i, n in enumerate(lengths):
        _compare(name, got, i, refs[(i, score_eos)], ORDER, n, n_best)
    # the fixture meets every kind of word: in the lexicon, hot, outside it, and unfinished at the end of the clip
    kinds = set()
    for i in range(len(lengths)):
        for pre, _, _, _ in refs[(i, score_eos)][0]:
            words = [tuple(g) for key, g in itertools.groupby(pre, lambda c: c == delim) if not key]
            kinds |= {"in" if w in k.lexicon else "out" for w in words}
            kinds |= {"pending"} if pre and pre[-1] != delim else set()
            kinds |= {"delimiter"} if delim in pre else set()
            kinds |= {"hot"} if any(w in k.hot for w in words) else set()
    assert kinds == {"in", "out", "hot", "pending", "delimiter"}, kinds


# ---- 2. exhaustive: scores are CTC likelihood + LM + word bonus + OOV scores + boosts -----------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("score_eos", [True, False], ids=["eos", "no-eos"])
def test_every_score_is_the_ctc_likelihood_plus_the_word_lm_plus_the_word_terms(score_eos):
    """3 non-blank classes (the delimiter and two letters), T = 3, beam 64: the 25 feasible label strings (1 + 3 + 9 + the 12 of three labels without a
    repeat, which would need a blank it has no frame for) never fill the beam, so nothing is pruned and the score of every hypothesis is its full CTC log-likelihood +
    alpha ln 10 LM(words, the pending word included) + beta (words) + oov_score (OOV words) + the boosts of its hot words (+ </s>)."""
    v, T, blank, delim, width, cap = 4, 3, 1, 2, 64, 3
    alpha, beta, oov, hot_w = 0.8, 0.6, -1.7, 1.1
    itos = _itos(v, blank, delim)                                             # letters: class 0 "a", class 3 "b"
    a, b = itos[0], itos[3]
    grams = {("<s>",): (-99.0, -0.3), ("</s>",): (-1.2, 0.0), ("<unk>",): (-2.0, 0.0), (a,): (-0.7, -0.2), (a + b,): (-1.1, -0.4), (b + a,): (-1.3, -0.1),
             ("<s>", a): (-0.4, -0.15), (a, a + b): (-0.6, -0.25), (a + b, "</s>"): (-0.5, 0.0), (a, a): (-0.9, -0.05), ("<s>", a, a + b): (-0.35, 0.0),
             (a, a, "</s>"): (-0.45, 0.0)}
    lexicon, hot = [a, a + b, b + a, b + b], [a + b, b + b]                  # "bb" is in the lexicon and not in the LM; "b" is outside both
    lm = _package_lm(itos, grams, lexicon, hot, 3, blank)
    k = _reference_words(itos, grams, lexicon, hot, {w: hot_w for w in hot}, 3, delim, alpha, beta, oov)
    x = _randn(177, (v, T), 1.5)
    ref = _search_word(x, blank, width, cap, k, score_eos)
    assert len(ref[0]) == 25
    got = _launch(torch.from_numpy(x)[None].contiguous(), T, blank, width, cap, 64, lm, (alpha, beta, oov, hot_w, None), score_eos)
    _compare("exhaustive", got, 0, ref, 3, T, 64)
    tokens, frames, lengths, scores, lm_scores, counts = got
    assert counts[0] == 25
    lp = _log_softmax64(x)
    worst = 0.0
    for n in range(25):
        s = tokens[0, n, : lengths[0, n]].tolist()
        words = [tuple(g) for key, g in itertools.groupby(s, lambda c: c == delim) if not key]
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
    print(f"RATIO|beam-word-lm-exhaustive-score|{worst:.3e}|T {T}, 25 strings")


# ---- 3. all weights zero is the search without an LM ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["v8-t50-w16-c7", "v70-t40-w16-c8", "b4-v8-t30-w8-c4-lengths"])
def test_with_every_weight_zero_it_agrees_with_the_plain_search(name):
    v, T, width, cap, blank, delim, lengths, _, _, _ = RANDOM[name]
    x, (itos, grams, lexicon, hot, _), _, _ = _random_case(name)
    lm = _package_lm(itos, grams, lexicon, hot, ORDER, blank)
    n_best = min(width, 8)
    free = _Words({}, 1, set(), {}, delim, 0.0, 0.0, 0.0)
    for i, n in enumerate(lengths):                                           # the plain search's own margin, on the weight-free reference
        _, gap, big = _search_word(x[i, :, :n], blank, width, cap, free, False)
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
TINY = ["<blank>", " ", "a", "c", "e", "o", "s", "t"]


def _c_vowel_t(first, second, third=None):
    """Seven frames that say c, blank, a vowel, blank, t, blank, blank; the vowel frame prefers `first` to `second` (to `third`) by half a logit."""
    x = -4.0 + 0.05 * _randn(5, (8, 7), 1.0)                                  # (the noise keeps the also-rans from tying)
    for t, c in enumerate([3, 0, None, 0, 7, 0, 0]):
        if c is not None:
            x[c, t] = 6.0
    x[TINY.index(first), 2], x[TINY.index(second), 2] = 5.5, 5.0
    if third:
        x[TINY.index(third), 2] = 4.5
    return x


def _texts(got):
    tokens, _, lengths, _, _, counts = got
    return ["".join(TINY[c] for c in tokens[0, n, : lengths[0, n]]) for n in range(int(counts[0]))]


@pytest.mark.gpu
def test_an_lm_that_prefers_cat_turns_cot_into_cat_and_a_hot_word_turns_it_back():
    from thunder_speech_amd.ctc_lm import WordNGramLM
    x = _c_vowel_t("o", "a")
    lg = torch.from_numpy(x)[None].contiguous()
    plain = _launch_plain(lg, 7, 0, 8, 4, 2)
    assert "".join(TINY[c] for c in plain[0][0, 0, : plain[2][0, 0]]) == "cot"
    lm = WordNGramLM.from_arpa(ARPA, TINY, 0, hotwords=["cot"])
    fused = _launch(lg, 7, 0, 8, 4, 2, lm, (1.0, 0.0, -10.0, 0.0, None), True)
    assert _texts(fused) == ["cat", "cot"]
    # <s> cat </s>: the bigram, then back-off(<s> cat) and the bigram; <s> cot </s>: both back off to the unigrams
    assert abs(float(fused[4][0, 0]) - (-0.7 - 0.1 - 0.8)) <= _tol(1.6) and abs(float(fused[4][0, 1]) - (-0.4 - 1.6 - 0.1 - 1.1)) <= _tol(3.2)
    assert _texts(_launch(lg, 7, 0, 8, 4, 2, lm, (0.0, 0.0, -10.0, 0.0, None), True))[0] == "cot"
    # the LM alone loses "cot" by 1.7 ln 10 - 0.5 = 3.4; a boost of 5 wins it back, and lm_scores do not see the boost
    hot = _launch(lg, 7, 0, 8, 4, 2, lm, (1.0, 0.0, -10.0, 5.0, None), True)
    assert _texts(hot) == ["cot", "cat"] and abs(float(hot[4][0, 0]) - (-0.4 - 1.6 - 0.1 - 1.1)) <= _tol(3.2)
    assert abs(float(hot[3][0, 0]) - (float(fused[3][0, 1]) + 5.0)) <= 2 * _tol(float(hot[3][0, 0]))
    assert _texts(_launch(lg, 7, 0, 8, 4, 2, lm, (1.0, 0.0, -10.0, 0.0, {"cot": 5.0}), True)) == ["cot", "cat"]


@pytest.mark.gpu
def test_a_large_negative_oov_score_keeps_an_out_of_lexicon_spelling_out_of_the_1_best():
    from thunder_speech_amd.ctc_lm import WordNGramLM
    x = _c_vowel_t("e", "a", "o")                                             # the acoustic model hears "cet", which is no word
    lg = torch.from_numpy(x)[None].contiguous()
    lm = WordNGramLM.from_arpa(ARPA, TINY, 0)
    assert _texts(_launch(lg, 7, 0, 8, 4, 3, lm, (0.0, 0.0, 0.0, 0.0, None), True))[0] == "cet"
    kept_out = _launch(lg, 7, 0, 8, 4, 3, lm, (0.0, 0.0, -20.0, 0.0, None), True)
    assert _texts(kept_out)[:2] == ["cat", "cot"] and "cet" not in _texts(kept_out)[:2]


# ---- 5. bookkeeping ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_captured_call_replays_the_eager_bits_and_a_new_setting_leaves_the_old_graph_alone():
    """WordNGramLM.weights gives a NEW cached setting for new boosts -- new word_factor / oov_factor tensors, nothing written at the old addresses
    -- so the graph captured under the old setting replays the old setting's bits."""
    name = "b4-v8-t30-w8-c4-lengths"
    v, T, width, cap, blank, delim, lengths, _, _, _ = RANDOM[name]
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
    assert w_new.tensors["edge_begin"].data_ptr() == w_old.tensors["edge_begin"].data_ptr()          # the trie does not depend on the setting
    other = _launch(torch.from_numpy(x), T, blank, width, cap, 4, lm, new, True, lengths)
    assert other[3].tobytes() != eager[3].tobytes()                           # the new boosts change scores
    for a, r in zip(eager, replay()):
        assert a.tobytes() == r.tobytes()                                     # the replay under the old setting is unchanged


@pytest.mark.gpu
def test_cells_beyond_lengths_and_counts_and_the_empty_clip():
    """T = 0 gives the empty hypothesis (no pending word; with </s> its score is alpha ln 10 log10 P(</s> | <s>)); a one-frame clip has as many
    hypotheses as it has candidates + 1, so ranks beyond stay empty: zero tokens, frames, lengths and lm_scores, -inf scores.  _launch pre-fills
    the workspace with 0xFF bytes and the outputs with garbage."""
    name = "b4-v8-t30-w8-c4-lengths"
    v, T, width, cap, blank, delim, lengths, _, _, _ = RANDOM[name]
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
def test_predict_beam_and_predict_nbest_with_a_word_lm_through_the_module():
    from thunder_speech_amd.ctc_lm import WordNGramLM
    from thunder_speech_amd.registry import load_pretrained
    module = load_pretrained("QuartzNet5x5_synthetic").cuda().eval()
    vocab = module.text_transform.vocab
    lm = WordNGramLM.from_arpa(ARPA, vocab.itos, vocab.blank_idx, hotwords=["dog"])
    assert lm.delimiter == vocab.itos.index(" ") and lm.dropped == 0
    rng = np.random.Generator(np.random.PCG64(7))
    x = torch.from_numpy((0.1 * rng.standard_normal((2, 16000))).astype(np.float32)).cuda()
    zero = dict(alpha=0.0, beta=0.0, oov_score=0.0, hotword_weight=0.0)
    assert module.predict_beam(x, beam_width=8, token_cap=4, lm=lm, **zero) == module.predict_beam(x, beam_width=8, token_cap=4)
    fused = module.predict_nbest(x, 3, beam_width=8, token_cap=4, lm=lm, alpha=0.5, beta=1.0, oov_score=-1.0, hotword_weight=2.0, boosts={"dog": 3.0})
    assert len(fused) == 2 and all(len(clip) >= 1 for clip in fused)
    for clip in fused:
        assert all(h0.score >= h1.score for h0, h1 in zip(clip, clip[1:]))
        for h in clip:
            ids = [vocab.itos.index(t.token) for t in h.tokens]
            want = lm.score(ids, eos=True)
            assert isinstance(h.lm_score, float) and abs(h.lm_score - want) <= _tol(want)
            assert h.text == module.text_transform._ids_to_text(ids)
    assert module.predict_beam(x, beam_width=8, token_cap=4, lm=lm) == [clip[0].text for clip in module.predict_nbest(x, 1, beam_width=8, token_cap=4, lm=lm)]
    other = WordNGramLM.from_arpa(ARPA, ["<blank>", "|"] + vocab.itos[1:-1] + [" "], 0, delimiter="|")       # another class ends its words
    with pytest.raises(ValueError, match="ends a word at class 1"):
        module.predict_beam(x, lm=other)
