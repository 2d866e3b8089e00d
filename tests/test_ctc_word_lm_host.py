"""Word-level n-gram fusion on the CPU: the open companion header include_open/thunder_speech_amd/ctc_beam_word_lm.h through `_lib.OPEN` and the built
library's symbols (COMPANIONS, STAGED and QUEUED untouched by it); WordNGramLM on the hand-written fixture tests/golden/lm_words_tiny.arpa -- the
trie, the words, the host lookup against a restatement over a plain set of spellings and the n-gram dictionary --; the tables of a setting; the
argument checks of the launcher (made-up pointers: none of these calls reaches a launch), the launch-config and workspace formulas, the refusal
of CPU tensors and of the lexicon keywords without a word LM."""
import ctypes
import glob
import itertools
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARPA = os.path.join(ROOT, "tests", "golden", "lm_words_tiny.arpa")
ITOS = ["<blank>", " ", "a", "c", "e", "o", "s", "t"]                         # the fixture's six letters; "dog" cannot be spelled
vp, i32, i64, cint = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int

NAMES = ["ts_ctc_beam_word_lm_abi_version", "ts_ctc_beam_word_lm_launch_config", "ts_ctc_beam_word_lm_workspace_bytes", "ts_ctc_beam_word_lm_search"]
FIELDS = [("n_nodes", i32), ("n_edges", i32), ("n_words", i32), ("delimiter", i32), ("unk_class", i32), ("edge_begin", vp), ("edge_class", vp),
          ("edge_next", vp), ("node_word", vp), ("word_class", vp), ("word_factor", vp), ("oov_factor", vp)]


# ---- 1. the binder -------------------------------------------------------------------------------------------------------------------------------
def test_open_header_parses_and_declares_exactly_its_names():
    from thunder_speech_amd import _lib
    assert "ctc_beam_word_lm" in _lib.OPEN
    h = _lib.OPEN["ctc_beam_word_lm"]
    assert h.path == os.path.join(ROOT, "include_open", "thunder_speech_amd", "ctc_beam_word_lm.h")
    assert list(h.signatures) == NAMES
    lm, lexicon = ctypes.POINTER(_lib.CtcLm), ctypes.POINTER(_lib.CtcLexicon)
    assert h.signatures["ts_ctc_beam_word_lm_abi_version"] == (cint, [])
    assert h.signatures["ts_ctc_beam_word_lm_launch_config"] == (cint, [i32, i32, i32, vp, vp, vp])
    assert h.signatures["ts_ctc_beam_word_lm_workspace_bytes"] == (i64, [i32, i32, i32, i32])
    assert h.signatures["ts_ctc_beam_word_lm_search"] == (cint, [vp, i32, i32, i32, i32, vp, i32, i32, i32, i32, i32, lm, lexicon, vp, vp, vp, vp, vp, vp, vp, vp])
    assert (h.version_define, h.version_function, h.abi_version) == ("TS_CTC_BEAM_WORD_LM_ABI_VERSION", "ts_ctc_beam_word_lm_abi_version", 1)
    assert list(h.structs) == ["ts_ctc_lexicon"] and h.structs["ts_ctc_lexicon"] is _lib.CtcLexicon and _lib.CtcLexicon._fields_ == FIELDS
    assert h.defines == {"TS_CTC_BEAM_WORD_LM_ABI_VERSION": 1}
    # the search takes the token-level search's arguments plus the lexicon
    assert [a for a in h.signatures["ts_ctc_beam_word_lm_search"][1] if a is not lexicon] == _lib.COMPANIONS["ctc_beam_lm"].signatures["ts_ctc_beam_lm_search"][1]
    others = [_lib.CORE, *_lib.COMPANIONS.values(), *_lib.STAGED.values(), *_lib.QUEUED.values(), *(o for k, o in _lib.OPEN.items() if k != "ctc_beam_word_lm")]
    assert not set().union(*(o.signatures for o in others)) & set(NAMES)


def test_a_struct_of_an_included_companion_is_known_and_an_unknown_one_is_an_error():
    from thunder_speech_amd import _lib
    text = "#define TS_Q_ABI_VERSION 1\nint ts_q_abi_version(void);\nint ts_q(const ts_ctc_lm* lm, const float* x);\n"
    sig, structs, _ = _lib.read_header(text, {"ts_ctc_lm": _lib.CtcLm})
    assert sig["ts_q"] == (cint, [ctypes.POINTER(_lib.CtcLm), vp]) and structs == {}
    with pytest.raises(ValueError, match="ts_ctc_lm"):
        _lib.read_header(text)


def test_companions_staged_and_queued_keep_their_keys():
    from thunder_speech_amd import _lib
    assert list(_lib.STAGED) == ["mxfp8"] and list(_lib.QUEUED) == ["lora_bank"]
    assert sorted(_lib.COMPANIONS) == sorted(os.path.basename(p)[:-2] for p in glob.glob(os.path.join(ROOT, "include", "thunder_speech_amd", "*.h")))
    assert not any("ctc_beam_word_lm" in table for table in (_lib.COMPANIONS, _lib.STAGED, _lib.QUEUED))
    assert _lib.SIGNATURES is _lib.CORE.signatures and not set(NAMES) & set(_lib.SIGNATURES) and _lib.ABI_VERSION == _lib.CORE.abi_version
    assert sorted(_lib.OPEN) == sorted(os.path.basename(p)[:-2] for p in glob.glob(os.path.join(ROOT, "include_open", "thunder_speech_amd", "*.h")))


def test_built_library_exports_the_names_and_reports_the_version():
    from thunder_speech_amd import _lib, build as b
    path = b.build(verbose=False)
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert not [n for n in NAMES if n not in defined]
    assert _lib.lib().ts_ctc_beam_word_lm_abi_version() == _lib.OPEN["ctc_beam_word_lm"].abi_version == 1


def test_editing_the_open_header_makes_the_library_stale(tmp_path, monkeypatch):
    from thunder_speech_amd import _lib, build as b
    header = _lib.OPEN["ctc_beam_word_lm"].path
    assert header in b.header_deps() and "-I" + os.path.join(ROOT, "include_open") in b.common_flags()
    lib = tmp_path / "lib.so"
    lib.write_bytes(b"")
    monkeypatch.setattr(b, "lib_path", lambda: str(lib))
    real = glob.glob
    monkeypatch.setattr(b, "sources", lambda: [])
    monkeypatch.setattr(b.glob, "glob", lambda pat, **kw: [p for p in real(pat, **kw) if p == header])
    mtime = os.path.getmtime(header)
    os.utime(lib, (mtime + 10, mtime + 10))
    assert not b.needs_build()
    os.utime(lib, (mtime - 10, mtime - 10))
    assert b.needs_build()


def test_the_kernel_source_keeps_the_shared_pre_pass_and_the_rounding_pragmas():
    csrc = os.path.join(ROOT, "thunder_speech_amd", "csrc")
    src = open(os.path.join(csrc, "ctc_beam_word_lm.hip")).read()
    assert '#include "ctc_beam_cand.hpp"' in src and "void ctc_beam_cand_kernel(" not in src and not re.search(r'#include\s+"[^"]*\.hip"', src)
    assert src.index("#pragma clang fp contract(off) reassociate(off)") < src.index('#include "ctc_beam_cand.hpp"')
    assert '#include "thunder_speech_amd/ctc_beam_word_lm.h"' in src
    code = re.sub(r"//[^\n]*", "", src)
    assert "atomic" not in code and not re.search(r"\b(exp|log|log10|pow)\s*\(\s*a\.", code)      # equal bits; no exp / log of a table on the device


# ---- 2. from_arpa --------------------------------------------------------------------------------------------------------------------------------
def _lm(**kw):
    from thunder_speech_amd.ctc_lm import WordNGramLM
    return WordNGramLM.from_arpa(ARPA, ITOS, 0, **kw)


def test_from_arpa_builds_the_trie_of_the_fixture():
    lm = _lm()
    words = ["a", "at", "cat", "cats", "coat", "cot", "eat", "oat", "sat", "seat", "set", "toe"]
    assert lm.order == 3 and lm.delimiter == 1 and lm.dropped == 1 and lm.dropped_ngrams == 3           # "dog": one word, three n-grams
    assert lm.lm_words == words and lm.words == words and lm.unk_class == 12 and lm.word_class == list(range(12)) and not any(lm.hot)
    assert lm.lm.n_classes == 14 and lm.lm.blank_idx == 13 and lm.lm.has_bos and lm.lm.has_eos and lm.lm.has_unk
    assert lm.lm.arcs[0][12] == (12, -1.5, 0)                                 # <unk>-as-a-word: <unk>'s unigram, leading to state 0
    assert [a[0] for a in lm.lm.arcs[0]] == list(range(13))                   # state 0: the whole unigram table and <unk>
    spell = lambda x: "".join(ITOS[c] for c in {v: k for k, v in lm.node_id.items()}[x])
    # every beginning of a word is a node, numbered by (length, classes); the terminal nodes are the words
    begins = sorted({w[:k] for w in words for k in range(len(w) + 1)}, key=lambda s: (len(s), [ITOS.index(ch) for ch in s]))
    assert [spell(x) for x in range(lm.n_nodes)] == begins and lm.n_nodes == 27
    assert {spell(x): lm.words[w] for x, w in enumerate(lm.node_word) if w >= 0} == {w: w for w in words}
    assert spell(0) == "" and lm.node_word[0] == -1 and [ITOS[c] for c, _ in lm.edges[0]] == ["a", "c", "e", "o", "s", "t"]
    for x, edges in enumerate(lm.edges):
        assert [c for c, _ in edges] == sorted({c for c, _ in edges})         # sorted by class, no class twice
        assert all(spell(nxt) == spell(x) + ITOS[c] for c, nxt in edges)
    assert sum(len(e) for e in lm.edges) == lm.n_nodes - 1


def test_from_arpa_hot_words_lexicon_and_spell():
    from thunder_speech_amd.ctc_lm import WordNGramLM
    hot = _lm(hotwords=["tea", "cat", "dog"])
    assert hot.words == sorted(_lm().words + ["tea"]) and hot.dropped == 1    # "dog" again: counted once
    assert [w for w, h in zip(hot.words, hot.hot) if h] == ["cat", "tea"]
    assert hot.word_class[hot.words.index("tea")] == hot.unk_class == 12      # a hot word the LM lacks is scored as <unk>
    assert hot.word_class[hot.words.index("cat")] == hot.lm_words.index("cat")
    small = _lm(lexicon=["cat", "a", "tees", "zebra"], hotwords=["cot"])
    assert small.words == ["a", "cat", "cot", "tees"] and small.dropped == 2 and small.hot == [False, False, True, False]   # "dog", "zebra"
    assert small.word_class == [small.lm_words.index("a"), small.lm_words.index("cat"), small.lm_words.index("cot"), small.unk_class]
    assert small.lm_words == _lm().lm_words                                   # the LM keeps its words whatever the lexicon
    up = WordNGramLM.from_arpa(ARPA, ["<pad>", "A", "C", "E", "O", "S", "T", "|"], 0, delimiter="|", spell=str.upper)
    assert up.words == _lm().words and up.delimiter == 7 and up.dropped == 1
    assert up.score([2, 1, 6, 7, 5, 1, 6], eos=True) == pytest.approx(_lm().score([3, 2, 7, 1, 6, 2, 7], eos=True))       # "cat sat"
    with pytest.raises(ValueError, match="no class"):
        WordNGramLM.from_arpa(ARPA, ITOS, 0, delimiter="|")
    with pytest.raises(ValueError, match="no class"):
        WordNGramLM.from_arpa(ARPA, ITOS, 1)                                  # the delimiter cannot be the blank
    with pytest.raises(ValueError, match="not hot words"):
        _lm(hotwords=["cot"]).weights(0.5, 1.0, boosts={"cat": 1.0}, device="cpu")


# ---- 3. the host lookup against a restatement ----------------------------------------------------------------------------------------------------
BOS, EOS, UNK, UNKW = "<s>", "</s>", "<unk>", "a word the LM does not know"


def _textbook(grams, order, hist, w, floor):
    """(log10 P(w | hist), fell to the floor) by the dictionary back-off over WORD STRINGS: the n-gram if the table has it, else
    back-off(context) + the same with a shorter context; a word without a unigram takes <unk>'s unigram or the floor."""
    total = 0.0
    ctx = tuple(hist[max(len(hist) - (order - 1), 0):]) if order > 1 else ()
    while True:
        if ctx + (w,) in grams:
            return total + grams[ctx + (w,)][0], False
        if not ctx:
            return total + (grams[(UNK,)][0] if (UNK,) in grams else floor), True
        total += grams.get(ctx, (0.0, 0.0))[1]
        ctx = ctx[1:]


def _restated(grams, order, lexicon, text, eos, floor):
    """(log10 LM score, OOV words, lexicon words) of a string of letters and spaces: split at the spaces, every word looked up by the textbook."""
    known = {w for g in grams for w in g}
    hist = (BOS,) if any(g[0] == BOS for g in grams) else ()
    total, oov, found = 0.0, 0, []
    for w in [w for w in text.split(" ") if w]:
        key = w if w in lexicon and w in known else UNKW
        oov += w not in lexicon
        found += [w] if w in lexicon else []
        p, fell = _textbook(grams, order, hist, key, floor)
        total, hist = total + p, (() if fell else hist + (key,))
    if eos and any(g[-1] == EOS for g in grams):
        total += _textbook(grams, order, hist, EOS, floor)[0]
    return total, oov, found


def _fixture_grams(without=()):
    """The fixture's n-grams as the ARPA text says them (read here, not by the package), less "dog" and the specials in `without`."""
    grams, section = {}, 0
    for line in open(ARPA).read().split("\\data\\")[1].splitlines():
        f = line.split()
        if line.startswith("\\"):
            section = int(line[1]) if line[1].isdigit() else 0
        elif section and f:
            gram = tuple(f[1:1 + section])
            if "dog" not in gram and not set(gram) & set(without):
                grams[gram] = (float(f[0]), float(f[1 + section]) if len(f) > 1 + section else 0.0)
    return grams


@pytest.mark.parametrize("without", [(), (BOS,), (EOS,), (UNK,), (BOS, EOS, UNK)], ids=["all", "no-bos", "no-eos", "no-unk", "none"])
def test_host_lookup_equals_the_restatement_over_every_short_label_string(without):
    """Every label string of up to 6 classes over the delimiter and the six letters, with and without </s>: score, OOV count and the lexicon's
    words met (hot ones among them) equal the restatement, which keeps the lexicon as a set of strings and reads the dictionary by the
    textbook back-off.  The lexicon leaves out some of the LM's words and holds two that the LM lacks."""
    from thunder_speech_amd.ctc_lm import WordNGramLM
    floor = -6.25
    grams = _fixture_grams(without)
    lexicon = ["a", "at", "cat", "cot", "eat", "oat", "sat", "set", "tea", "ace"]                  # "tea", "ace": not in the LM; no "cats", "coat", ...
    lm = WordNGramLM(3, grams, ITOS, 0, " ", lexicon, ["cot", "tea"], None, floor)
    if not without:                                                           # from_arpa reads the same LM from the file ("dog" dropped there)
        same = WordNGramLM.from_arpa(ARPA, ITOS, 0, lexicon=lexicon, hotwords=["cot", "tea"], unk_log10=floor)
        assert same.lm.grams == lm.lm.grams and same.lm.arcs == lm.lm.arcs and same.edges == lm.edges and same.word_class == lm.word_class
    assert (lm.lm.has_bos, lm.lm.has_eos, lm.lm.has_unk) == (BOS not in without, EOS not in without, UNK not in without)
    assert {g for g in grams if len(g) == 1 and g[0] not in (BOS, EOS, UNK)} == {(w,) for w in lm.lm_words if (w,) in grams}
    n = 0
    for length in range(7):
        for labels in itertools.product(range(1, 8), repeat=length):
            s = "".join(ITOS[c] for c in labels)
            for eos in (False, True):
                want, oov, found = _restated(grams, 3, set(lexicon), s, eos, floor)
                got, got_oov, got_words = lm.walk(labels, eos)
                assert got == pytest.approx(want, abs=1e-12) and got_oov == oov and [lm.words[w] for w in got_words] == found, (s, eos)
                assert lm.score(labels, eos) == got
            n += 1
    assert n == sum(7 ** k for k in range(7))
    # step by step: the pair (state, x) after a string is that of its words, and x says where the pending word stands
    s, x = lm.start_state, 0
    for ch, (want_x, oov) in zip("cat tx ", [("c", 0), ("ca", 0), ("cat", 0), ("", 0), ("t", 0), (None, 1), ("", 0)]):
        r = lm.step(s, x, ITOS.index(ch) if ch != "x" else 6)                 # "ts": no word begins so
        s, x = r.state, r.x
        assert r.oov == bool(oov) and (x == -1 if want_x is None else x == lm.node_id[tuple(ITOS.index(c) for c in want_x)])
    assert lm.finish(s, 0) == (0.0, s, 0, False, None) and lm.step(s, 0, 1) == lm.finish(s, 0)     # a doubled delimiter changes nothing
    with pytest.raises(ValueError):
        lm.step(s, 0, 0)


# ---- 4. the tables of a setting ------------------------------------------------------------------------------------------------------------------
def test_weights_tables_are_formed_on_the_host_per_setting():
    lm = _lm(hotwords=["cot", "tea"])
    t = lm.lexicon_tables(oov_score=-3.0, hotword_weight=1.5, boosts={"tea": 4.0})
    n, e, w = lm.n_nodes, lm.n_nodes - 1, len(lm.words)
    assert all(t[k].dtype == np.int32 for k in ("edge_begin", "edge_class", "edge_next", "node_word", "word_class"))
    assert t["word_factor"].dtype == t["oov_factor"].dtype == np.float64
    assert {k: v.shape for k, v in t.items()} == {"edge_begin": (n + 1,), "edge_class": (e,), "edge_next": (e,), "node_word": (n,), "word_class": (w,),
                                                  "word_factor": (w,), "oov_factor": (1,)}
    assert t["edge_begin"][0] == 0 and t["edge_begin"][-1] == e
    for x in range(n):
        lo, hi = t["edge_begin"][x], t["edge_begin"][x + 1]
        assert list(zip(t["edge_class"][lo:hi].tolist(), t["edge_next"][lo:hi].tolist())) == lm.edges[x]
    assert t["node_word"].tolist() == lm.node_word and t["word_class"].tolist() == lm.word_class
    want = [math.exp(4.0) if x == "tea" else math.exp(1.5) if x == "cot" else 1.0 for x in lm.words]
    np.testing.assert_array_equal(t["word_factor"], np.exp(np.array([4.0 if x == "tea" else 1.5 if x == "cot" else 0.0 for x in lm.words])))
    assert t["word_factor"].tolist() == pytest.approx(want) and t["oov_factor"].tolist() == [math.exp(-3.0)]
    a = lm.lm.tables(0.7, 1.5)                                                # the word automaton's factors are NGramLM.tables'
    np.testing.assert_array_equal(a["arc_factor"], np.power(10.0, 0.7 * a["arc_log10"]) * math.exp(1.5))
    z, za = lm.lexicon_tables(0.0, 0.0), lm.lm.tables(0.0, 0.0)
    assert (z["word_factor"] == 1.0).all() and (z["oov_factor"] == 1.0).all()
    assert (za["arc_factor"] == 1.0).all() and (za["bo_factor"] == 1.0).all() and (za["eos_factor"] == 1.0).all()
    assert lm.word_boosts(1.5, {"tea": 4.0}) == tuple(4.0 if x == "tea" else 1.5 if x == "cot" else 0.0 for x in lm.words)


# ---- 5. the launcher -----------------------------------------------------------------------------------------------------------------------------
def _structs(lm_over, lx_over):
    from thunder_speech_amd import _lib
    A = 0x20000
    lm = dict(n_states=3, n_arcs=7, start_state=1, has_eos=1, arc_begin=A, arc_class=A, arc_next=A, arc_factor=A, arc_log10=A, bo_next=A, bo_factor=A,
              bo_log10=A, eos_factor=A, eos_log10=A)
    lx = dict(n_nodes=5, n_edges=4, n_words=2, delimiter=1, unk_class=2, edge_begin=A, edge_class=A, edge_next=A, node_word=A, word_class=A,
              word_factor=A, oov_factor=A)
    lm.update(lm_over)
    lx.update(lx_over)
    return _lib.CtcLm(**lm), _lib.CtcLexicon(**lx)


def _host_cases():
    """(entry point, arguments, expected status) of calls that return before any launch.  Pointers are made-up addresses (never dereferenced on
    these paths): A is 16-byte aligned.  `lm` / `lx`: fields of the two structs to override, or None for a NULL struct."""
    A, E, U = 0x10000, -1, -2
    bs = lambda lg=A, b=2, v=8, t=50, pitch=64, il=A, blank=0, w=16, cap=4, nb=2, eos=1, lm={}, lx={}, tok=A, fr=A, ln=A, sc=A, lsc=A, cnt=A, ws=A: (
        "ts_ctc_beam_word_lm_search", (lg, b, v, t, pitch, il, blank, w, cap, nb, eos, lm, lx, tok, fr, ln, sc, lsc, cnt, ws, None))
    wb = lambda b=2, t=50, w=16, cap=4: ("ts_ctc_beam_word_lm_workspace_bytes", (b, t, w, cap))
    cases = [
        (bs(lg=0), E), (bs(tok=0), E), (bs(fr=0), E), (bs(ln=0), E), (bs(sc=0), E), (bs(lsc=0), E), (bs(cnt=0), E), (bs(ws=0), E), (bs(lm=None), E),
        (bs(lx=None), E),
        (bs(b=0), E), (bs(b=-1), E), (bs(v=0), E), (bs(t=0), E), (bs(t=-1), E), (bs(pitch=49), E), (bs(blank=-1), E), (bs(blank=8), E),
        (bs(w=0), E), (bs(cap=0), E), (bs(nb=0), E), (bs(w=-1), E), (bs(cap=-1), E), (bs(nb=-1), E), (bs(nb=17), E), (bs(w=1, nb=2), E),
        (bs(w=65), U), (bs(cap=65), U), (bs(w=64, nb=65, v=4), U), (bs(w=65, nb=65), U), (bs(w=1000, cap=1000, nb=1), U),
        (bs(ws=A + 8), U), (bs(ws=A + 4), U), (bs(v=(1 << 24) + 1, pitch=64), U),
        # the 1024-candidate limit: beam_width (min(token_cap, n_classes - 1) + 1)
        (bs(v=32, w=64, cap=16), U), (bs(v=32, w=64, cap=64), U), (bs(v=40, w=61, cap=16), U), (bs(v=40, w=33, cap=31), U),
        # the word automaton
        (bs(lm=dict(arc_begin=0)), E), (bs(lm=dict(arc_class=0)), E), (bs(lm=dict(arc_next=0)), E), (bs(lm=dict(arc_factor=0)), E),
        (bs(lm=dict(arc_log10=0)), E), (bs(lm=dict(bo_next=0)), E), (bs(lm=dict(bo_factor=0)), E), (bs(lm=dict(bo_log10=0)), E),
        (bs(lm=dict(eos_factor=0)), E), (bs(lm=dict(eos_log10=0)), E), (bs(lm=dict(n_states=0)), E), (bs(lm=dict(n_arcs=-1)), E),
        (bs(lm=dict(start_state=3)), E), (bs(lm=dict(start_state=-1)), E),
        (bs(lm=dict(arc_factor=0x20004)), U), (bs(lm=dict(bo_log10=0x20004)), U), (bs(lm=dict(eos_factor=0x20004)), U),
        # the lexicon
        (bs(lx=dict(edge_begin=0)), E), (bs(lx=dict(edge_class=0)), E), (bs(lx=dict(edge_next=0)), E), (bs(lx=dict(node_word=0)), E),
        (bs(lx=dict(word_class=0)), E), (bs(lx=dict(word_factor=0)), E), (bs(lx=dict(oov_factor=0)), E),
        (bs(lx=dict(n_nodes=0)), E), (bs(lx=dict(n_nodes=-1)), E), (bs(lx=dict(n_edges=-1)), E), (bs(lx=dict(n_words=-1)), E),
        (bs(lx=dict(delimiter=-1)), E), (bs(lx=dict(delimiter=8)), E), (bs(lx=dict(delimiter=0)), E), (bs(blank=1), E),      # the delimiter is the blank
        (bs(lx=dict(word_factor=0x20004)), U), (bs(lx=dict(oov_factor=0x20004)), U), (bs(lx=dict(oov_factor=0x20001)), U),
        (wb(b=0), E), (wb(t=0), E), (wb(w=0), E), (wb(cap=0), E), (wb(w=65), U), (wb(cap=65), U),
    ]
    return [(name, args, want) for (name, args), want in cases]


@pytest.mark.parametrize("name,args,want", _host_cases(), ids=lambda v: v if isinstance(v, str) and v.startswith("ts_") else None)
def test_launcher_refuses_bad_arguments_before_any_launch(name, args, want):
    from thunder_speech_amd import _lib
    assert (_lib.TS_EINVAL, _lib.TS_EUNSUPPORTED) == (-1, -2)
    keep = None
    if name == "ts_ctc_beam_word_lm_search":
        lm, lx = args[11], args[12]
        keep = _structs(lm or {}, lx or {})
        args = args[:11] + (None if lm is None else ctypes.byref(keep[0]), None if lx is None else ctypes.byref(keep[1])) + args[13:]
    assert getattr(_lib.lib(), name)(*args) == want


def _query(L, n_classes, width, cap):
    out = [ctypes.c_int32(-7) for _ in range(3)]
    st = L.ts_ctc_beam_word_lm_launch_config(n_classes, width, cap, *[ctypes.addressof(o) for o in out])
    return st, tuple(o.value for o in out)


def _expected(n_classes, width, cap):
    """The header's formulas: threads, LDS bytes, candidates."""
    cap = min(cap, n_classes - 1)
    cands = width * (cap + 1)
    up = lambda x, m: (x + m - 1) // m * m
    return up(cands, 64), 96 * up(width, 8) + 16 * up(cands, 8) + 48 * up(cap + 2, 2) + 2064, cands


@pytest.mark.parametrize("n_classes,width,cap", [(29, 16, 8), (32, 64, 15), (1025, 32, 31), (1025, 1, 1), (3, 64, 2), (2, 1, 1), (1, 4, 4), (29, 1, 64),
                                                 (5, 7, 3), (7, 8, 3), (70, 16, 8), (16, 64, 64), (1 << 24, 15, 64)])
def test_launch_config_follows_the_header_formulas(n_classes, width, cap):
    from thunder_speech_amd import _lib
    st, got = _query(_lib.lib(), n_classes, width, cap)
    assert st == 0 and got == _expected(n_classes, width, cap)
    threads, lds, cands = got
    assert cands <= threads <= 1024 and lds <= 28 * 1024


def test_launch_config_refusals_and_the_workspace_formula():
    from thunder_speech_amd import _lib
    L = _lib.lib()
    assert _query(L, 32, 64, 15) == (0, (1024, 96 * 64 + 16 * 1024 + 48 * 18 + 2064, 1024))       # the largest workgroup there is
    for bad, want in (((0, 16, 8), -1), ((29, 0, 8), -1), ((29, 16, 0), -1), ((29, 65, 8), -2), ((29, 16, 65), -2), (((1 << 24) + 1, 16, 8), -2),
                      ((32, 64, 16), -2), ((17, 61, 16), -2), ((1025, 33, 31), -2), ((1025, 64, 64), -2)):
        assert _query(L, *bad)[0] == want
    assert _query(L, 16, 64, 16)[0] == 0                                      # the clamped cap counts: 64 (15 + 1)
    out = ctypes.c_int32(0)
    assert L.ts_ctc_beam_word_lm_launch_config(29, 16, 8, None, ctypes.addressof(out), ctypes.addressof(out)) == -1
    f = lambda b, t, w, cap: b * (32 * (t * w + 1) + 12 * t * (cap + 2) + 512 * t + 768)
    for args in ((1, 1, 1, 1), (16, 999, 16, 8), (16, 999, 64, 15), (64, 751, 64, 64), (3, 37, 7, 3)):
        assert L.ts_ctc_beam_word_lm_workspace_bytes(*args) == f(*args)
    assert L.ts_ctc_beam_word_lm_workspace_bytes(70000, 70000, 64, 64) == f(70000, 70000, 64, 64) > 2 ** 32    # 64-bit arithmetic


def test_cpu_tensors_are_refused():
    from thunder_speech_amd.ctc_lm import WordNGramLM, beam_search_word_lm
    from thunder_speech_amd.registry import load_pretrained
    module = load_pretrained("QuartzNet5x5_synthetic")
    vocab = module.text_transform.vocab
    lm = WordNGramLM.from_arpa(ARPA, vocab.itos, vocab.blank_idx, hotwords=["dog"])
    assert lm.dropped == 0 and lm.delimiter == vocab.itos.index(" ")
    assert lm.score([vocab.itos.index(ch) for ch in "a cat"], eos=True) == pytest.approx(-0.4 + -0.2 + -0.5)          # <s> a cat </s>, all highest order
    x = torch.zeros(1, 4000)
    with pytest.raises(RuntimeError, match=r"GPU tensors required \(no CPU fallback\)"):
        module.predict_beam(x, lm=lm, hotword_weight=2.0)
    with pytest.raises(RuntimeError, match=r"GPU tensors required \(no CPU fallback\)"):
        module.predict_nbest(x, 3, lm=lm, alpha=0.3, beta=0.5, oov_score=-2.0, boosts={"dog": 1.0})
    small = _lm()
    with pytest.raises(RuntimeError, match=r"beam_search_word_lm: GPU tensors required \(no CPU fallback\)"):
        beam_search_word_lm(torch.zeros(1, 8, 9), small, 0.5, 1.0)
    with pytest.raises(RuntimeError, match=r"WordNGramLM.weights: GPU tensors required \(no CPU fallback\)"):
        small.weights(0.5, 1.0, device="cpu")


# ---- 6. the module's keywords --------------------------------------------------------------------------------------------------------------------
def test_lexicon_keywords_without_a_word_lm_are_value_errors():
    from thunder_speech_amd.ctc_lm import NGramLM, WordNGramLM
    from thunder_speech_amd.registry import load_pretrained
    module = load_pretrained("QuartzNet5x5_synthetic")
    vocab = module.text_transform.vocab
    token_lm = NGramLM.from_arpa(os.path.join(ROOT, "tests", "golden", "lm_tiny.arpa"), vocab.itos, vocab.blank_idx)
    x = torch.zeros(1, 4000)
    for kw in (dict(hotword_weight=1.0), dict(oov_score=-3.0), dict(boosts={"cat": 1.0})):
        for lm in (token_lm, None):
            with pytest.raises(ValueError, match="WordNGramLM"):
                module.predict_beam(x, lm=lm, **kw)
            with pytest.raises(ValueError, match="WordNGramLM"):
                module.predict_nbest(x, 2, lm=lm, **kw)
    # a word LM whose words end at another class than the one this vocabulary shows as " "
    other = WordNGramLM.from_arpa(ARPA, ["|"] + vocab.itos[1:], vocab.blank_idx, delimiter="a")
    with pytest.raises(ValueError, match="ends a word at class 1"):
        module.predict_beam(x, lm=other)
