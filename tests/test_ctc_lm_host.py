"""N-gram shallow fusion on the CPU: the ARPA reader, the back-off automaton of thunder_speech_amd/ctc_lm.py against the textbook dictionary
back-off, the pre-pass shared with the search without an LM, the argument checks of the launcher (made-up pointers: none of these calls
reaches a launch), the launch-config and workspace formulas, and the refusal of CPU tensors.  (The companion C header:
tests/test_abi_headers_host.py.)"""
import ctypes
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARPA = os.path.join(ROOT, "tests", "golden", "lm_tiny.arpa")
ITOS = ["<blank>", "a", "c", "o", "t", "x"]                                  # "x" has no unigram in the fixture: an OOV class


# ---- the ARPA reader -----------------------------------------------------------------------------------------------------------------------------
def test_read_arpa_on_the_hand_written_fixture():
    from thunder_speech_amd.ctc_lm import read_arpa
    order, tables = read_arpa(ARPA)
    assert order == 3 and [len(t) for t in tables] == [8, 9, 6]
    assert tables[0][("<unk>",)] == (-1.2, 0.0) and tables[0][("<s>",)] == (-99.0, -0.4)
    assert tables[0][("t",)] == (-0.6, 0.0)                                   # a lower-order line without its back-off reads as 0
    assert tables[0][("o",)] == (-0.9, -0.2)                                  # spaces and tabs mixed
    assert tables[1][("c", "o")] == (-1.4, -0.1) and tables[1][("o", "t")] == (-0.9, 0.0)
    assert tables[2][("o", "t", "</s>")] == (-1.3, 0.0) and tables[2][("<s>", "c", "a")] == (-0.1, 0.0)
    assert read_arpa(open(ARPA).read()) == (order, tables)                    # the text itself


GOOD = "\\data\\\nngram 1=2\nngram 2=1\n\n\\1-grams:\n-1.0\ta\t-0.5\n-1.0\tb\n\n\\2-grams:\n-0.3\ta b\n\n\\end\\\n"


@pytest.mark.parametrize("bad,line", [
    (GOOD.replace("-0.3\ta b", "-0.3\ta b\t-0.1"), 10),                        # a back-off at the highest order
    (GOOD.replace("-1.0\tb", "-1.0"), 7),                                     # a line without its word
    (GOOD.replace("-1.0\tb", "minus\tb"), 7),                                 # not a number
    (GOOD.replace("-1.0\tb", "-1.0\tb\tnan"), 7),
    (GOOD.replace("ngram 2=1", "ngram two=1"), 3),
    (GOOD.replace("\\2-grams:", "\\3-grams:"), 9),                            # a section nobody announced
    (GOOD.replace("\\2-grams:", "\\two-grams:"), 9),
    (GOOD.replace("-1.0\tb", "-1.0\ta"), 7),                                  # the same n-gram twice
    (GOOD.replace("\\end\\\n", ""), 11),                                       # no end marker
    (GOOD.replace("ngram 1=2", "ngram 1=3"), 12),                             # a count that does not hold
    (GOOD + "-1.0\tc\n", 13),                                                 # text after the end
    (GOOD.replace("\\data\\", "\\dada\\"), 1),
])
def test_read_arpa_names_the_line_of_malformed_input(bad, line):
    from thunder_speech_amd.ctc_lm import read_arpa
    assert read_arpa(GOOD)[0] == 2
    with pytest.raises(ValueError, match=rf"line {line}\b"):
        read_arpa(bad)


def test_from_arpa_matches_words_to_classes():
    from thunder_speech_amd.ctc_lm import BOS, EOS, UNK, NGramLM
    lm = NGramLM.from_arpa(ARPA, ITOS, 0)
    assert lm.order == 3 and lm.dropped == 2 and lm.has_bos and lm.has_eos and lm.has_unk          # "z" and "z q" match no class
    assert lm.contexts[0] == () and lm.contexts[lm.start_state] == (BOS,)
    assert (2, 1, 4) in lm.grams and (BOS, 2, 1) in lm.grams and (1, 4, EOS) in lm.grams and (UNK,) in lm.grams
    assert [a[0] for a in lm.arcs[0]] == [1, 2, 3, 4, 5]                       # every class but the blank, sorted
    assert lm.arcs[0][4] == (5, -1.2, 0)                                      # the OOV class takes <unk>'s unigram and leads to state 0
    assert lm.score([2, 1, 4], eos=True) == pytest.approx(-0.3 + -0.1 + -0.15 + -0.2)              # <s> c a t </s>, all highest order
    assert lm.score([2, 3, 4], eos=True) == pytest.approx(-0.3 + (-0.15 + -1.4) + -1.6 + -1.3)     # <s> c o: backs off from (<s>, c)
    assert lm.score([2, 1, 4], eos=True) > lm.score([2, 3, 4], eos=True)
    with pytest.raises(ValueError):
        lm.step(0, 0)                                                         # the blank never has an LM id
    # a blank elsewhere, and a map from the LM's words to the model's tokens
    up = NGramLM.from_arpa(ARPA, ["A", "C", "<blank>", "O", "T"], 2, token_of=str.upper)
    assert up.dropped == 2 and up.score([1, 0, 4], eos=True) == pytest.approx(lm.score([2, 1, 4], eos=True))
    # classes that spell the LM's specials are not LM words
    w2v = NGramLM.from_arpa(ARPA, ["<pad>", "<s>", "</s>", "<unk>", "a", "c", "o", "t"], 0)
    assert w2v.arcs[0][0] == (1, -1.2, 0) and w2v.score([5, 4, 7]) == pytest.approx(lm.score([2, 1, 4]))
    no_unk = NGramLM.from_arpa(open(ARPA).read().replace("-1.2\t<unk>\n", "").replace("ngram 1=8", "ngram 1=7"), ITOS, 0, unk_log10=-7.5)
    assert not no_unk.has_unk and no_unk.arcs[0][4] == (5, -7.5, 0)


# ---- the automaton against the textbook ----------------------------------------------------------------------------------------------------------
def _textbook(grams, order, hist, w, unk_id, floor):
    """(log10 P(w | hist), fell to the floor) by the dictionary back-off: the n-gram if the table has it, else back-off(context) + the same with a
    shorter context; a word without a unigram takes <unk>'s unigram or the floor."""
    total = 0.0
    ctx = tuple(hist[max(len(hist) - (order - 1), 0):]) if order > 1 else ()
    while True:
        if ctx + (w,) in grams:
            return total + grams[ctx + (w,)][0], False
        if not ctx:
            return total + (grams[(unk_id,)][0] if (unk_id,) in grams else floor), True
        total += grams.get(ctx, (0.0, 0.0))[1]
        ctx = ctx[1:]


def _random_grams(rng, order, words, bos, eos, unk, keep=0.5):
    grams = {}
    for n in range(1, order + 1):
        for g in itertools.product(words, repeat=n):
            if bos in g[1:] or eos in g[:-1] or (unk in g and n > 1):
                continue
            if rng.random() < keep:
                grams[g] = (float(rng.uniform(-3, -0.1)), float(rng.uniform(-1, 0)) if n < order and g[-1] != eos else 0.0)
    return grams


@pytest.mark.parametrize("with_bos,with_eos,with_unk", list(itertools.product([False, True], repeat=3)))
def test_automaton_lookup_equals_the_textbook_back_off(with_bos, with_eos, with_unk):
    """V = 5 (a blank, three LM words, one OOV class), order 3, a sparse table that is not prefix-closed: every context of up to 3 classes, from
    the start state and from state 0, every next class and </s>.  After a class that took the floor the context is empty (the next state is 0)."""
    from thunder_speech_amd.ctc_lm import BOS, EOS, UNK, NGramLM
    order, floor = 3, -6.25
    for seed in range(6):
        rng = np.random.Generator(np.random.PCG64(1000 + seed))
        words = [1, 2, 3] + [BOS] * with_bos + [EOS] * with_eos + [UNK] * with_unk
        grams = _random_grams(rng, order, words, BOS, EOS, UNK)
        if with_bos:
            grams.setdefault((BOS, 1), (-0.5, -0.25))
        if with_eos:
            grams.setdefault((2, EOS), (-0.75, 0.0))
        if with_unk:
            grams.setdefault((UNK,), (-2.5, 0.0))
        lm = NGramLM(order, grams, 5, 0, unk_log10=floor)
        assert (lm.has_bos, lm.has_eos, lm.has_unk) == (with_bos, with_eos, with_unk)
        assert lm.contexts[0] == () and all(lm.backoff[s][1] < s for s in range(1, lm.n_states))
        assert all([a[0] for a in arcs] == sorted({a[0] for a in arcs}) for arcs in lm.arcs)     # sorted by class, no class twice
        assert lm.start_state == (lm.state_id[(BOS,)] if with_bos else 0)
        for length in range(4):
            for ctx in itertools.product([1, 2, 3, 4], repeat=length):
                for from_start in ([True, False] if with_bos else [False]):
                    s, hist = (lm.start_state, (BOS,)) if from_start else (0, ())
                    for c in ctx:
                        got, s = lm.step(s, c)
                        want, fell = _textbook(grams, order, hist, c, UNK, floor)
                        assert got == pytest.approx(want, abs=1e-12)
                        hist = () if fell else hist + (c,)
                    for w in (1, 2, 3, 4):
                        assert lm.step(s, w)[0] == pytest.approx(_textbook(grams, order, hist, w, UNK, floor)[0], abs=1e-12), (seed, ctx, from_start, w)
                    want_eos = _textbook(grams, order, hist, EOS, UNK, floor)[0] if with_eos else 0.0
                    assert lm.eos(s) == pytest.approx(want_eos, abs=1e-12)


def test_weights_tables_are_formed_on_the_host_per_setting():
    from thunder_speech_amd.ctc_lm import NGramLM
    lm = NGramLM.from_arpa(ARPA, ITOS, 0)
    t = lm.tables(0.7, 1.5)
    n = lm.n_states
    assert t["arc_begin"].dtype == np.int32 and t["arc_begin"].shape == (n + 1,) and t["arc_begin"][0] == 0 and t["arc_begin"][-1] == len(t["arc_class"])
    assert all(t[k].dtype == np.float64 for k in ("arc_factor", "arc_log10", "bo_factor", "bo_log10", "eos_factor", "eos_log10"))
    assert all(t[k].shape == (n,) for k in ("bo_next", "bo_factor", "bo_log10", "eos_factor", "eos_log10"))
    for s in range(n):
        lo, hi = t["arc_begin"][s], t["arc_begin"][s + 1]
        assert [(int(c), float(p), int(nx)) for c, p, nx in zip(t["arc_class"][lo:hi], t["arc_log10"][lo:hi], t["arc_next"][lo:hi])] == lm.arcs[s]
    np.testing.assert_array_equal(t["arc_factor"], np.power(10.0, 0.7 * t["arc_log10"]) * math.exp(1.5))
    np.testing.assert_array_equal(t["bo_factor"], np.power(10.0, 0.7 * t["bo_log10"]))
    np.testing.assert_array_equal(t["eos_factor"], np.power(10.0, 0.7 * t["eos_log10"]))          # </s> carries no beta
    z = lm.tables(0.0, 0.0)
    assert (z["arc_factor"] == 1.0).all() and (z["bo_factor"] == 1.0).all() and (z["eos_factor"] == 1.0).all()


# ---- the sources ---------------------------------------------------------------------------------------------------------------------------------
def test_the_candidate_pre_pass_is_shared_through_a_header():
    csrc = os.path.join(ROOT, "thunder_speech_amd", "csrc")
    beam, fused, shared = (open(os.path.join(csrc, n)).read() for n in ("ctc_beam.hip", "ctc_beam_lm.hip", "ctc_beam_cand.hpp"))
    assert shared.count("void ctc_beam_cand_kernel(") == 1
    for src in (beam, fused):
        assert '#include "ctc_beam_cand.hpp"' in src and "void ctc_beam_cand_kernel(" not in src and not re.search(r'#include\s+"[^"]*\.hip"', src)
        assert src.index("#pragma clang fp contract(off) reassociate(off)") < src.index('#include "ctc_beam_cand.hpp"')
    assert '#include "thunder_speech_amd/ctc_beam_lm.h"' in fused and "ts_ctc_beam_lm" not in beam
    assert "atomic" not in re.sub(r"//[^\n]*", "", fused)                     # equal arguments give equal bits


# ---- argument checks -----------------------------------------------------------------------------------------------------------------------------
def _lm_struct(**over):
    from thunder_speech_amd import _lib
    A = 0x20000
    f = dict(n_states=3, n_arcs=7, start_state=1, has_eos=1, arc_begin=A, arc_class=A, arc_next=A, arc_factor=A, arc_log10=A, bo_next=A, bo_factor=A,
             bo_log10=A, eos_factor=A, eos_log10=A)
    f.update(over)
    return _lib.CtcLm(**f)


def _host_cases():
    """(entry point, arguments, expected status) of calls that return before any launch.  Pointers are made-up addresses (never dereferenced on
    these paths): A is 16-byte aligned."""
    A, E, U = 0x10000, -1, -2
    LM = "default"
    bs = lambda lg=A, b=2, v=8, t=50, pitch=64, il=A, blank=0, w=16, cap=4, nb=2, eos=1, lm=LM, tok=A, fr=A, ln=A, sc=A, lsc=A, cnt=A, ws=A: (
        "ts_ctc_beam_lm_search", (lg, b, v, t, pitch, il, blank, w, cap, nb, eos, lm, tok, fr, ln, sc, lsc, cnt, ws, None))
    wb = lambda b=2, t=50, w=16, cap=4: ("ts_ctc_beam_lm_workspace_bytes", (b, t, w, cap))
    cases = [
        (bs(lg=0), E), (bs(tok=0), E), (bs(fr=0), E), (bs(ln=0), E), (bs(sc=0), E), (bs(lsc=0), E), (bs(cnt=0), E), (bs(ws=0), E), (bs(lm=None), E),
        (bs(b=0), E), (bs(b=-1), E), (bs(v=0), E), (bs(t=0), E), (bs(t=-1), E), (bs(pitch=49), E), (bs(blank=-1), E), (bs(blank=8), E),
        (bs(w=0), E), (bs(cap=0), E), (bs(nb=0), E), (bs(w=-1), E), (bs(cap=-1), E), (bs(nb=-1), E), (bs(nb=17), E), (bs(w=1, nb=2), E),
        (bs(w=65), U), (bs(cap=65), U), (bs(w=64, nb=65, v=4), U), (bs(w=65, nb=65), U), (bs(w=1000, cap=1000, nb=1), U),
        (bs(ws=A + 8), U), (bs(ws=A + 4), U), (bs(v=(1 << 24) + 1, pitch=64), U),
        # the 1024-candidate limit: beam_width (min(token_cap, n_classes - 1) + 1)
        (bs(v=32, w=64, cap=16), U), (bs(v=32, w=64, cap=64), U), (bs(v=40, w=61, cap=16), U), (bs(v=40, w=33, cap=31), U),
        (bs(lm=dict(arc_begin=0)), E), (bs(lm=dict(arc_class=0)), E), (bs(lm=dict(arc_next=0)), E), (bs(lm=dict(arc_factor=0)), E),
        (bs(lm=dict(arc_log10=0)), E), (bs(lm=dict(bo_next=0)), E), (bs(lm=dict(bo_factor=0)), E), (bs(lm=dict(bo_log10=0)), E),
        (bs(lm=dict(eos_factor=0)), E), (bs(lm=dict(eos_log10=0)), E), (bs(lm=dict(n_states=0)), E), (bs(lm=dict(n_arcs=-1)), E),
        (bs(lm=dict(start_state=3)), E), (bs(lm=dict(start_state=-1)), E),
        (bs(lm=dict(arc_factor=0x20004)), U), (bs(lm=dict(bo_log10=0x20004)), U), (bs(lm=dict(eos_factor=0x20004)), U),
        (wb(b=0), E), (wb(t=0), E), (wb(w=0), E), (wb(cap=0), E), (wb(w=65), U), (wb(cap=65), U),
    ]
    return [(name, args, want) for (name, args), want in cases]


@pytest.mark.parametrize("name,args,want", _host_cases(), ids=lambda v: v if isinstance(v, str) and v.startswith("ts_") else None)
def test_launcher_refuses_bad_arguments_before_any_launch(name, args, want):
    from thunder_speech_amd import _lib
    assert (_lib.TS_EINVAL, _lib.TS_EUNSUPPORTED) == (-1, -2)
    keep = None
    if name == "ts_ctc_beam_lm_search":
        lm = args[11]
        keep = None if lm is None else _lm_struct(**({} if lm == "default" else lm))
        args = args[:11] + (None if keep is None else ctypes.byref(keep),) + args[12:]
    assert getattr(_lib.lib(), name)(*args) == want


# ---- the launch-config query and the workspace ---------------------------------------------------------------------------------------------------
def _query(L, n_classes, width, cap):
    out = [ctypes.c_int32(-7) for _ in range(3)]
    st = L.ts_ctc_beam_lm_launch_config(n_classes, width, cap, *[ctypes.addressof(o) for o in out])
    return st, tuple(o.value for o in out)


def _expected(n_classes, width, cap):
    """The header's formulas: candidates, threads, LDS bytes."""
    cap = min(cap, n_classes - 1)
    cands = width * (cap + 1)
    up = lambda x, m: (x + m - 1) // m * m
    return up(cands, 64), 88 * up(width, 8) + 16 * up(cands, 8) + 48 * up(cap + 2, 2) + 2064, cands


@pytest.mark.parametrize("n_classes,width,cap", [(29, 16, 8), (32, 64, 15), (1025, 32, 31), (1025, 1, 1), (3, 64, 2), (2, 1, 1), (1, 4, 4), (29, 1, 64),
                                                 (5, 7, 3), (7, 8, 3), (40, 16, 8), (16, 64, 64), (1 << 24, 15, 64)])
def test_launch_config_follows_the_header_formulas(n_classes, width, cap):
    from thunder_speech_amd import _lib
    st, got = _query(_lib.lib(), n_classes, width, cap)
    assert st == 0 and got == _expected(n_classes, width, cap)
    threads, lds, cands = got
    assert cands <= threads <= 1024 and lds <= 28 * 1024


def test_launch_config_at_the_limits_and_its_refusals():
    from thunder_speech_amd import _lib
    L = _lib.lib()
    assert L.ts_ctc_beam_lm_abi_version() == 1
    assert _query(L, 32, 64, 15) == (0, (1024, 88 * 64 + 16 * 1024 + 48 * 18 + 2064, 1024))       # the largest workgroup there is
    assert _query(L, 29, 16, 8)[1] == (192, 88 * 16 + 16 * 144 + 48 * 10 + 2064, 144)
    for bad, want in (((0, 16, 8), -1), ((29, 0, 8), -1), ((29, 16, 0), -1), ((29, 65, 8), -2), ((29, 16, 65), -2), (((1 << 24) + 1, 16, 8), -2),
                      ((32, 64, 16), -2), ((17, 61, 16), -2), ((1025, 33, 31), -2), ((1025, 64, 64), -2)):
        assert _query(L, *bad)[0] == want
    assert _query(L, 16, 64, 16)[0] == 0                                      # the clamped cap counts: 64 (15 + 1)
    out = ctypes.c_int32(0)
    assert L.ts_ctc_beam_lm_launch_config(29, 16, 8, None, ctypes.addressof(out), ctypes.addressof(out)) == -1


def test_workspace_formula():
    from thunder_speech_amd import _lib
    L = _lib.lib()
    f = lambda b, t, w, cap: b * (32 * (t * w + 1) + 12 * t * (cap + 2) + 512 * t + 768)
    for args in ((1, 1, 1, 1), (16, 999, 16, 8), (16, 999, 64, 15), (64, 751, 64, 64), (3, 37, 7, 3)):
        assert L.ts_ctc_beam_lm_workspace_bytes(*args) == f(*args)
    assert L.ts_ctc_beam_lm_workspace_bytes(70000, 70000, 64, 64) == f(70000, 70000, 64, 64) > 2 ** 32    # 64-bit arithmetic


# ---- no CPU path ---------------------------------------------------------------------------------------------------------------------------------
def test_cpu_tensors_are_refused():
    from thunder_speech_amd.ctc_lm import NGramLM, beam_search_lm
    from thunder_speech_amd.registry import load_pretrained
    module = load_pretrained("QuartzNet5x5_synthetic")
    vocab = module.text_transform.vocab
    lm = NGramLM.from_arpa(ARPA, vocab.itos, vocab.blank_idx)
    assert lm.score([vocab.itos.index(ch) for ch in "cat"], eos=True) == pytest.approx(-0.3 + -0.1 + -0.15 + -0.2)
    x = torch.zeros(1, 4000)
    with pytest.raises(RuntimeError, match=r"GPU tensors required \(no CPU fallback\)"):
        module.predict_beam(x, lm=lm)
    with pytest.raises(RuntimeError, match=r"GPU tensors required \(no CPU fallback\)"):
        module.predict_nbest(x, 3, lm=lm, alpha=0.3, beta=0.5)
    small = NGramLM.from_arpa(ARPA, ITOS, 0)
    with pytest.raises(RuntimeError, match=r"beam_search_lm: GPU tensors required \(no CPU fallback\)"):
        beam_search_lm(torch.zeros(1, 6, 9), small, 0.5, 1.0)
    with pytest.raises(RuntimeError, match=r"GPU tensors required \(no CPU fallback\)"):
        small.weights(0.5, 1.0, "cpu")


def test_hypothesis_gains_a_trailing_lm_score():
    from thunder_speech_amd.ctc_beam import BeamToken, Hypothesis, hypotheses_from_tables
    assert Hypothesis("a", -1.0, []) == Hypothesis("a", -1.0, [], None) and Hypothesis("a", -1.0).lm_score is None
    itos = ["<blank>", "h", "i"]
    tokens, frames = np.array([[[1, 2, 0]]], np.int32), np.array([[[0, 2, 0]]], np.int32)
    args = (tokens, frames, np.array([[2]], np.int32), np.array([[-0.5]], np.float32), np.array([1], np.int32), itos, lambda ids: "".join(itos[i] for i in ids), 320, 16000)
    assert hypotheses_from_tables(*args)[0][0] == Hypothesis("hi", -0.5, [BeamToken("h", 0, 0.0), BeamToken("i", 2, 0.04)])
    got = hypotheses_from_tables(*args, np.array([[-1.25]], np.float32))[0][0]
    assert got.lm_score == -1.25 and isinstance(got.lm_score, float) and got.text == "hi"
