"""CTC prefix beam search with n-gram shallow fusion on the GPU (include/thunder_speech_amd/ctc_beam_lm.h, csrc/ctc_beam_lm.hip) through the raw C
ABI and through the module.

The reference is `_search_lm` below: the header's algorithm restated in float64 in the LOG domain, in the style of `_search` of
tests/test_gpu_ctc_beam.py, with prefixes as tuples (no hashes, no trie, no automaton): the LM score of a token is read from the n-gram DICTIONARY
by the textbook back-off (`_textbook`), the context being the tokens so far (emptied by a token that took the floor of a word without a unigram).
Nothing of the package takes part in it.  Independent of that restatement, the exhaustive case compares every score with
CTC log-likelihood (plain float64 alpha recursion) + alpha ln 10 LM(labels) + beta len (+ alpha ln 10 LM(</s>)).

Tolerance of a score and of an lm_score: 2^-23 max(1, |value|) -- the one f32 rounding (2^-24 relative) plus float64 noise.

The margin condition (asserted by every test that demands equal tokens) is that of tests/test_gpu_ctc_beam.py with the LM's roundings added to
its count of fewer than 32 ulp per frame and side.  Per frame the fused search adds to a mass, on the device: at most N - 1 back-off products and
one arc product (N the LM's order), each by a factor that carries up to 3 ulp of its own (a product, a power and an exponential on the host)
-- 4 N ulp relative; in the reference: at most N sums for the token's log10 score, two products (alpha, ln 10) and two sums (beta, the mass)
-- N + 4 roundings, each an ABSOLUTE error of an ulp of the magnitude of its partial sum, which is at most max(M, L), M the largest |log key|
and L the largest |alpha ln 10 log10 p + beta| of a token.  Fewer than 32 + 4 N + 4 <= 32 + 8 N ulp per frame on either side (the one </s>
product per utterance is covered by the slack of the first term), adding up linearly over the T frames: two log keys closer than
E = (64 + 16 N) T 2^-53 max(1, M, L) may fall either way, and the tests require the smallest gap (last kept key against first dropped key over
all frames, and neighbouring keys of the final beam after </s>) to exceed E.  The fixtures' margins were measured on the CPU before the
seeds were fixed (>= 1e-7 against E ~ 1e-11); the assertion stays in every test.

Ratios error / bound are printed as `RATIO|kind|ratio|case`."""
import functools
import itertools
import math
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARPA = os.path.join(ROOT, "tests", "golden", "lm_tiny.arpa")
NEG = float("-inf")
U53 = 2.0 ** -53
LN10 = math.log(10.0)
BOS, EOS, UNK = -1, -2, -3                                                   # ids of <s>, </s>, <unk> inside the n-gram dictionaries
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


def _lm_of(grams, order, labels, eos):
    """log10 P(labels [</s>]) from <s> (if the dictionary has it): token by token, in forward order."""
    hist = (BOS,) if any(g[0] == BOS for g in grams) else ()
    total = 0.0
    for c in labels:
        p, fell = _textbook(grams, order, hist, c)
        total += p
        hist = () if fell else hist + (c,)
    if eos and any(g[-1] == EOS for g in grams):
        total += _textbook(grams, order, hist, EOS)[0]
    return total


def _search_lm(x, blank, width, cap, grams, order, alpha, beta, eos):
    """x [V, T] f32 -> (final beam [(prefix, frames, log key, log10 LM score)], smallest decision gap, largest magnitude): the header, word by word."""
    V, T = x.shape
    cap = min(cap, V - 1)
    has_eos = any(g[-1] == EOS for g in grams)
    start = (BOS,) if any(g[0] == BOS for g in grams) else ()
    beam = [((), (), 0.0, NEG, start, 0.0)]                                # prefix, frames, p_b, p_nb, LM context, log10 LM score so far
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
                lp, fell = _textbook(grams, order, hist, c)
                w = alpha * LN10 * lp + beta
                big = max(big, abs(w))
                mass = (pb if pre and pre[-1] == c else tot) + p[c] + w
                if pre + (c,) in slot:
                    j = slot[pre + (c,)]
                    stay[j][1] = _ladd(stay[j][1], mass)
                else:
                    children.append((pre + (c,), fr + (t,), NEG, mass, () if fell else hist + (c,), lm10 + lp))
        allc = [(e[0], e[1], s[0], s[1], e[4], e[5]) for e, s in zip(beam, stay)] + children
        keys = [_ladd(c[2], c[3]) for c in allc]
        order_ = [k for k in sorted(range(len(allc)), key=lambda k: (-keys[k], k)) if keys[k] != NEG]
        if len(order_) > width:
            gap = min(gap, keys[order_[width - 1]] - keys[order_[width]])
        beam = [allc[k] for k in order_[:width]]
        big = max([big] + [abs(keys[k]) for k in order_[:width]])
    final = []
    for pre, fr, pb, pnb, hist, lm10 in beam:
        key = _ladd(pb, pnb)
        if eos and has_eos:
            lp = _textbook(grams, order, hist, EOS)[0]
            key, lm10 = key + alpha * LN10 * lp, lm10 + lp
            big = max(big, abs(alpha * LN10 * lp), abs(key))
        final.append((pre, fr, key, lm10))
    final = [final[k] for k in sorted(range(len(final)), key=lambda k: (-final[k][2], k))]
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


# ---- LMs -----------------------------------------------------------------------------------------------------------------------------------------
def _random_grams(seed, v, blank, order, oov, common, with_bos=True, with_eos=True, with_unk=True, per_order=1500):
    """A random sparse n-gram dictionary over the classes but `blank` and `oov` (which gets no unigram): about half of the possible n-grams of an
    order, or `per_order` of them where that is fewer, log10 p in [-3, -0.1], back-offs in [-1, 0].  With many classes the words of the longer
    n-grams come mostly from `common` (the classes the logits prefer), so that the search meets them.  Not prefix-closed."""
    rng = np.random.Generator(np.random.PCG64(seed))
    words = [c for c in range(v) if c not in (blank, oov)]
    grams = {}
    val = lambda n, last: (float(rng.uniform(-3.0, -0.1)), float(rng.uniform(-1.0, 0.0)) if n < order and last != EOS else 0.0)
    for n in range(1, order + 1):
        possible = len(words) ** n
        if possible <= 2 * per_order:
            for g in itertools.product(words, repeat=n):
                if rng.random() < 0.5:
                    grams[g] = val(n, g[-1])
        else:
            for _ in range(per_order):
                g = tuple(int(rng.choice(common)) if rng.random() < 0.85 else int(rng.choice(words)) for _ in range(n))
                grams[g] = val(n, g[-1])
        if n >= 2:                                                          # some of them start a sentence, some end one
            for g in [g for g in grams if len(g) == n - 1 and g[0] >= 0 and g[-1] >= 0]:
                if with_bos and rng.random() < 0.3:
                    grams[(BOS,) + g] = val(n, g[-1])
                if with_eos and rng.random() < 0.3:
                    grams[g + (EOS,)] = val(n, EOS)
    for c in common[:2]:
        grams.setdefault((c,), val(1, c))
    if with_bos:
        grams[(BOS,)] = (-99.0, float(rng.uniform(-1.0, 0.0)))
    if with_eos:
        grams[(EOS,)] = val(1, EOS)
    if with_unk:
        grams[(UNK,)] = val(1, EOS)
    assert not any(oov in g for g in grams)
    return grams


def _package_lm(grams, order, v, blank):
    from thunder_speech_amd.ctc_lm import BOS as B, EOS as E, UNK as U, NGramLM
    assert (B, E, U) == (BOS, EOS, UNK)
    return NGramLM(order, grams, v, blank, unk_log10=FLOOR)


# ---- the launch ----------------------------------------------------------------------------------------------------------------------------------
def _launch(logits, n_frames, blank, width, cap, n_best, lm, alpha, beta, eos, lengths=None, graph=False):
    """logits: CPU f32 [B, V, pitch]; lm: the package's NGramLM.  Returns numpy (tokens, frames, lengths, scores, lm_scores, counts)."""
    import ctypes
    from thunder_speech_amd import _lib
    L = _lib.lib()
    b, v, pitch = logits.shape
    lg = logits.cuda()
    il = None if lengths is None else torch.tensor(lengths, dtype=torch.int32).cuda()
    w = lm.weights(alpha, beta)
    nbytes = L.ts_ctc_beam_lm_workspace_bytes(b, n_frames, width, cap)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    i32 = lambda *s: torch.full(s, -7, dtype=torch.int32, device="cuda")
    f32 = lambda *s: torch.full(s, 7.0, dtype=torch.float32, device="cuda")
    out = [i32(b, n_best, n_frames), i32(b, n_best, n_frames), i32(b, n_best), f32(b, n_best), f32(b, n_best), i32(b)]

    def call():
        st = L.ts_ctc_beam_lm_search(lg.data_ptr(), b, v, n_frames, pitch, None if il is None else il.data_ptr(), blank, width, cap, n_best, int(eos),
                                     ctypes.byref(w.struct), *[o.data_ptr() for o in out], ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert st == 0, st

    if not graph:
        call()
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in out]
    call()
    torch.cuda.synchronize()
    eager = [o.cpu().numpy().copy() for o in out]
    for o in out:
        o.fill_(-9)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            call()
    for o in out:
        o.fill_(-9)
    g.replay()
    torch.cuda.synchronize()
    return eager, [o.cpu().numpy() for o in out]


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
    return (64 + 16 * order) * max(T, 1) * U53 * max(1.0, big)


def _compare(name, got, i, ref, order, T, n_best):
    """Utterance i of `got` against the reference result `ref`: margin, then tokens, frames, lengths, counts equal, scores and lm_scores within
    the tolerance."""
    tokens, frames, lengths, scores, lm_scores, counts = got
    final, gap, big = ref
    e = _bound(order, T, big)
    print(f"RATIO|beam-lm-margin|{e / gap if gap < math.inf else 0.0:.3e}|{name}[{i}] E / smallest decision gap (E {e:.3e}, gap {gap:.3e})")
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
    print(f"RATIO|beam-lm-score|{worst:.3e}|{name}[{i}] (T {T}, {len(want)} hypotheses)")


def _randn(seed, shape, scale=3.0):
    return (scale * np.random.Generator(np.random.PCG64(seed)).standard_normal(shape)).astype(np.float32)


# ---- 1. random cases against the reference -------------------------------------------------------------------------------------------------------
RANDOM = {  # name: B, V, T, order, beam_width, token_cap, blank, lengths, (with <s>, </s>, <unk>), alpha, beta, seed
    "b3-v7-t40-o3-w8-c3": (3, 7, 40, 3, 8, 3, 0, [40, 27, 1], (True, True, True), 0.7, 0.9, 0),
    "b2-v40-t60-o5-w16-c8": (2, 40, 60, 5, 16, 8, 39, [60, 41], (True, True, False), 0.5, 1.0, 1),
    "b1-v32-t30-o4-w64-c15": (1, 32, 30, 4, 64, 15, 0, [27], (False, True, True), 0.9, 0.5, 2),      # 64 (15 + 1) = 1024 candidates: the limit
    "b1-v5-t20-o2-w1-c1": (1, 5, 20, 2, 1, 1, 2, [17], (False, False, False), 1.3, -0.4, 3),
}


@functools.lru_cache(maxsize=None)
def _random_case(name):
    """The logits [B, V, pitch] (pitch > T, NaN in every cell beyond a length), the dictionary and per (utterance, eos) the reference: computed once."""
    b, v, T, order, width, cap, blank, lengths, (bos, eos, unk), alpha, beta, seed = RANDOM[name]
    classes = [c for c in range(v) if c != blank]
    common = classes[: min(6, len(classes))]
    oov = common[1]                                                       # a class the logits prefer and the LM does not know
    grams = _random_grams(500 + seed, v, blank, order, oov, [c for c in common if c != oov], bos, eos, unk)
    x = np.full((b, v, T + 9), np.nan, np.float32)
    for i in range(b):
        x[i, :, : lengths[i]] = _randn(50 + 10 * seed + i, (v, lengths[i]))
        x[i, common, : lengths[i]] += 2.0
    refs = {(i, e): _search_lm(x[i, :, : lengths[i]], blank, width, cap, grams, order, alpha, beta, e) for i in range(b) for e in (False, True)}
    return x, grams, refs


@pytest.mark.gpu
@pytest.mark.parametrize("score_eos", [True, False], ids=["eos", "no-eos"])
@pytest.mark.parametrize("name", list(RANDOM))
def test_equals_the_reference_where_the_margin_condition_holds(name, score_eos):
    b, v, T, order, width, cap, blank, lengths, _, alpha, beta, _ = RANDOM[name]
    x, grams, refs = _random_case(name)
    lm = _package_lm(grams, order, v, blank)
    n_best = min(width, 8)
    got = _launch(torch.from_numpy(x), T, blank, width, cap, n_best, lm, alpha, beta, score_eos, lengths)
    for i in range(b):
        _compare(name, got, i, refs[(i, score_eos)], order, lengths[i], n_best)
    used = {c for i in range(b) for pre, _, _, _ in refs[(i, score_eos)][0] for c in pre}
    assert name.endswith("w1-c1") or [c for c in used if (c,) not in grams]   # an OOV class made it into a final hypothesis


# ---- 2. exhaustive: scores are CTC likelihood + LM + bonus ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("score_eos", [True, False], ids=["eos", "no-eos"])
def test_every_score_is_the_ctc_likelihood_plus_the_lm_score_plus_the_bonus(score_eos):
    """V = 4, T = 6, beam 64, all three labels candidates in every frame.  Up to the fifth frame every feasible string fits the beam (61 at most);
    the fifth frame prunes, which costs a final hypothesis mass only if it was dropped there and came back in the last frame -- the fixture's
    last frame is a near-certain blank, so the 64 survivors of the fifth frame stay (asserted on the reference: no final token at the last
    frame), and the score of every hypothesis is its full CTC log-likelihood + alpha ln 10 LM + beta len."""
    v, T, blank, width, cap, order, alpha, beta = 4, 6, 1, 64, 3, 3, 0.8, 0.6
    x = _randn(77, (v, T))
    x[blank, T - 1] += 30.0
    grams = _random_grams(78, v, blank, order, 3, [0, 2])
    lm = _package_lm(grams, order, v, blank)
    ref = _search_lm(x, blank, width, cap, grams, order, alpha, beta, score_eos)
    final = ref[0]
    assert len(final) == 64 and all(T - 1 not in fr for _, fr, _, _ in final)
    got = _launch(torch.from_numpy(x)[None].contiguous(), T, blank, width, cap, 64, lm, alpha, beta, score_eos)
    _compare("exhaustive", got, 0, ref, order, T, 64)
    tokens, frames, lengths, scores, lm_scores, counts = got
    lp = _log_softmax64(x)
    worst = 0.0
    for n in range(64):
        s = tokens[0, n, : lengths[0, n]].tolist()
        lm10 = _lm_of(grams, order, s, score_eos)
        want = _ctc_ll(lp, s, blank) + alpha * LN10 * lm10 + beta * len(s)
        worst = max(worst, abs(float(scores[0, n]) - want) / _tol(want))
        assert abs(float(scores[0, n]) - want) <= _tol(want), f"rank {n} {s}: {scores[0, n]!r} against {want!r}"
        assert abs(float(lm_scores[0, n]) - lm10) <= _tol(lm10)
    print(f"RATIO|beam-lm-exhaustive-score|{worst:.3e}|T {T}, 64 strings")


# ---- 3. alpha = beta = 0 is the search without an LM ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["b2-v40-t60-o5-w16-c8", "b1-v32-t30-o4-w64-c15"])
def test_without_weight_and_bonus_it_agrees_with_the_plain_search(name):
    b, v, T, order, width, cap, blank, lengths, _, _, _, _ = RANDOM[name]
    x, grams, _ = _random_case(name)
    lm = _package_lm(grams, order, v, blank)
    n_best = min(width, 8)
    for i in range(b):                                                        # the plain search's own margin (tests/test_gpu_ctc_beam.py), on the LM-free reference
        _, gap, big = _search_lm(x[i, :, : lengths[i]], blank, width, cap, {}, 1, 0.0, 0.0, False)
        assert gap > _bound(order, lengths[i], big)
    plain = _launch_plain(torch.from_numpy(x), T, blank, width, cap, n_best, lengths)
    for eos in (True, False):
        tokens, frames, out_len, scores, lm_scores, counts = _launch(torch.from_numpy(x), T, blank, width, cap, n_best, lm, 0.0, 0.0, eos, lengths)
        assert tokens.tobytes() == plain[0].tobytes() and frames.tobytes() == plain[1].tobytes()
        assert out_len.tobytes() == plain[2].tobytes() and counts.tobytes() == plain[4].tobytes()
        for a, p in zip(scores.reshape(-1), plain[3].reshape(-1)):
            assert abs(float(a) - float(p)) <= _tol(float(p))
        for i in range(b):                                                    # the LM is still reported
            for n in range(int(counts[i])):
                want = _lm_of(grams, order, tokens[i, n, : out_len[i, n]].tolist(), eos)
                assert abs(float(lm_scores[i, n]) - want) <= _tol(want)


# ---- 4. behaviour: the LM changes the answer -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_an_lm_that_prefers_cat_turns_cot_into_cat():
    from thunder_speech_amd.ctc_lm import NGramLM
    itos = ["<blank>", "a", "c", "o", "t", "x"]
    x = -4.0 + 0.05 * _randn(5, (6, 7), 1.0)                                  # (the noise keeps the also-rans from tying)
    for t, c in enumerate([2, 0, None, 0, 4, 0, 0]):
        if c is not None:
            x[c, t] = 6.0
    x[3, 2], x[1, 2] = 5.5, 5.0                                             # the acoustic model hears "o" a little better than "a"
    lm = NGramLM.from_arpa(ARPA, itos, 0)
    lg = torch.from_numpy(x)[None].contiguous()
    text = lambda tok, ln: "".join(itos[c] for c in tok[0, 0, : ln[0, 0]])
    plain = _launch_plain(lg, 7, 0, 8, 4, 2)
    assert text(plain[0], plain[2]) == "cot"
    tokens, frames, lengths, scores, lm_scores, counts = _launch(lg, 7, 0, 8, 4, 2, lm, 1.0, 0.0, True)
    assert text(tokens, lengths) == "cat" and "".join(itos[c] for c in tokens[0, 1, : lengths[0, 1]]) == "cot"
    assert abs(float(lm_scores[0, 0]) - (-0.3 - 0.1 - 0.15 - 0.2)) <= _tol(0.75) and abs(float(lm_scores[0, 1]) - (-0.3 - 0.15 - 1.4 - 1.6 - 1.3)) <= _tol(4.75)
    ref = _search_lm(x, 0, 8, 4, {g: v for g, v in lm.grams.items()}, 3, 1.0, 0.0, True)
    _compare("cat", (tokens, frames, lengths, scores, lm_scores, counts), 0, ref, 3, 7, 2)
    unweighted = _launch(lg, 7, 0, 8, 4, 2, lm, 0.0, 0.0, True)
    assert text(unweighted[0], unweighted[2]) == "cot"


# ---- 5. bookkeeping ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_captured_call_replays_the_eager_bits_and_two_calls_agree():
    name = "b3-v7-t40-o3-w8-c3"
    b, v, T, order, width, cap, blank, lengths, _, alpha, beta, _ = RANDOM[name]
    x, grams, _ = _random_case(name)
    lm = _package_lm(grams, order, v, blank)
    eager, replay = _launch(torch.from_numpy(x), T, blank, width, cap, 4, lm, alpha, beta, True, lengths, graph=True)
    again = _launch(torch.from_numpy(x), T, blank, width, cap, 4, lm, alpha, beta, True, lengths)
    for a, r, c in zip(eager, replay, again):
        assert a.tobytes() == r.tobytes() == c.tobytes()
    assert eager[5].tolist() == [4, 4, 4]                                     # the one-frame clip: the empty string and its three single tokens


@pytest.mark.gpu
def test_cells_beyond_lengths_and_counts_and_the_empty_clip():
    """T = 0 gives the empty hypothesis (with </s>: its score is alpha ln 10 log10 P(</s> | <s>)); a one-frame clip over three classes has three
    hypotheses, so ranks beyond stay empty: zero tokens, frames, lengths and lm_scores, -inf scores."""
    v, n, blank, width, cap, n_best, order, alpha, beta = 3, 12, 0, 8, 2, 6, 2, 0.6, 0.3
    grams = {(1,): (-0.5, -0.2), (2,): (-0.9, -0.1), (BOS,): (-99.0, -0.3), (BOS, 1): (-0.4, 0.0), (EOS,): (-1.1, 0.0), (BOS, EOS): (-2.0, 0.0), (1, EOS): (-0.25, 0.0)}
    lm = _package_lm(grams, order, v, blank)
    lengths = [0, 1, n]
    x = np.full((3, v, n + 4), np.nan, np.float32)
    for i, T in enumerate(lengths):
        x[i, :, :T] = _randn(90 + i, (v, T))
    for eos in (True, False):
        got = _launch(torch.from_numpy(x), n, blank, width, cap, n_best, lm, alpha, beta, eos, lengths)
        for i, T in enumerate(lengths):
            _compare(f"edges-eos{int(eos)}", got, i, _search_lm(x[i, :, :T], blank, width, cap, grams, order, alpha, beta, eos), order, T, n_best)
        tokens, frames, out_len, scores, lm_scores, counts = got
        assert counts.tolist() == [1, 3, n_best]
        assert out_len[0, 0] == 0 and abs(float(scores[0, 0]) - (alpha * LN10 * -2.0 if eos else 0.0)) <= _tol(1.0)
        assert abs(float(lm_scores[0, 0]) - (-2.0 if eos else 0.0)) <= _tol(2.0)
        assert (scores[0, 1:] == NEG).all() and (scores[1, 3:] == NEG).all() and not lm_scores[0, 1:].any() and not lm_scores[1, 3:].any()
        assert not out_len[0].any() and not out_len[1, 3:].any() and not tokens[0].any() and not frames[0].any() and not tokens[1, 3:].any()
    clamped = _launch(torch.from_numpy(x), n, blank, width, cap, n_best, lm, alpha, beta, True, [-3, 1, n + 50])
    for a, c in zip(_launch(torch.from_numpy(x), n, blank, width, cap, n_best, lm, alpha, beta, True, lengths), clamped):
        assert a.tobytes() == c.tobytes()                                      # lengths outside [0, n_frames] are clamped


# ---- 6. through the module -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_predict_beam_and_predict_nbest_with_an_lm_through_the_module():
    from thunder_speech_amd.ctc_lm import NGramLM
    from thunder_speech_amd.registry import load_pretrained
    module = load_pretrained("QuartzNet5x5_synthetic").cuda().eval()
    vocab = module.text_transform.vocab
    lm = NGramLM.from_arpa(ARPA, vocab.itos, vocab.blank_idx)
    rng = np.random.Generator(np.random.PCG64(7))
    x = torch.from_numpy((0.1 * rng.standard_normal((2, 16000))).astype(np.float32)).cuda()
    assert module.predict_beam(x, beam_width=8, token_cap=4, lm=lm, alpha=0.0, beta=0.0) == module.predict_beam(x, beam_width=8, token_cap=4)
    plain = module.predict_nbest(x, 3, beam_width=8, token_cap=4)
    assert all(h.lm_score is None for clip in plain for h in clip)
    fused = module.predict_nbest(x, 3, beam_width=8, token_cap=4, lm=lm, alpha=0.5, beta=1.0)
    assert len(fused) == 2 and all(len(clip) >= 1 for clip in fused)
    for clip in fused:
        assert all(h0.score >= h1.score for h0, h1 in zip(clip, clip[1:]))
        for h in clip:
            want = lm.score([vocab.itos.index(t.token) for t in h.tokens], eos=True)
            assert isinstance(h.lm_score, float) and abs(h.lm_score - want) <= _tol(want)
            assert h.text == module.text_transform._ids_to_text([vocab.itos.index(t.token) for t in h.tokens])
    assert module.predict_beam(x, beam_width=8, token_cap=4, lm=lm) == [clip[0].text for clip in module.predict_nbest(x, 1, beam_width=8, token_cap=4, lm=lm)]
