"""Word-level n-gram fusion for sentencepiece vocabularies on the CPU: the open companion header include_open/thunder_speech_amd/ctc_beam_piece_lm.h
through `_lib.OPEN` (it includes another open companion and takes its struct) and the built library's symbols; PieceWordNGramLM on the hand-written
fixture tests/golden/lm_words_tiny.arpa and a small piece vocabulary over its six letters -- every segmentation of a word reaches one trie node and
one score, the walk over pieces equals WordNGramLM's walk over the same text in a character vocabulary, where the OOV factor is paid, what a bare
U+2581 piece and a class without a spelling do --; the piece tables; the argument checks of the launcher (made-up pointers: none of these calls
reaches a launch), the launch-config and workspace formulas; the module's refusal of an LM compiled for another vocabulary."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARPA = os.path.join(ROOT, "tests", "golden", "lm_words_tiny.arpa")
PIECES = ["<blank>", "<unk>", "▁", "▁a", "▁c", "▁ca", "▁cat", "▁s", "a", "c", "e", "o", "s", "t", "at"]
CHARS = ["<blank>", " ", "a", "c", "e", "o", "s", "t"]                       # the character vocabulary of tests/test_ctc_word_lm_host.py
vp, i32, i64, cint = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int

NAMES = ["ts_ctc_beam_piece_lm_abi_version", "ts_ctc_beam_piece_lm_launch_config", "ts_ctc_beam_piece_lm_workspace_bytes", "ts_ctc_beam_piece_lm_search"]
FIELDS = [("n_classes", i32), ("n_letters", i32), ("n_piece_letters", i32), ("piece_begin", vp), ("piece_letter", vp), ("piece_kind", vp)]


def _ids(*pieces):
    return [PIECES.index(p) for p in pieces]


def _lm(**kw):
    from thunder_speech_amd.ctc_lm import PieceWordNGramLM
    return PieceWordNGramLM.from_arpa(ARPA, PIECES, 0, **kw)


def _char_lm(**kw):
    from thunder_speech_amd.ctc_lm import WordNGramLM
    return WordNGramLM.from_arpa(ARPA, CHARS, 0, **kw)


def _segmentations(word):
    """Every way to write `word` in PIECES: a piece that starts a word (or the bare word start), then pieces that continue it."""
    def rest(s):
        if not s:
            return [[]]
        return [[p] + r for p in PIECES[8:] if s.startswith(p) for r in rest(s[len(p):])]
    return [[p] + r for p in PIECES[2:8] if word.startswith(p[1:]) for r in rest(word[len(p) - 1:])]


# ---- 1. the binder -------------------------------------------------------------------------------------------------------------------------------
def test_open_header_parses_with_the_struct_of_the_open_header_it_includes():
    from thunder_speech_amd import _lib
    h = _lib.OPEN["ctc_beam_piece_lm"]
    assert h.path == os.path.join(ROOT, "include_open", "thunder_speech_amd", "ctc_beam_piece_lm.h")
    assert list(h.signatures) == NAMES
    lm, lexicon, pieces = ctypes.POINTER(_lib.CtcLm), ctypes.POINTER(_lib.CtcLexicon), ctypes.POINTER(_lib.CtcPieces)
    assert h.signatures["ts_ctc_beam_piece_lm_abi_version"] == (cint, [])
    assert h.signatures["ts_ctc_beam_piece_lm_launch_config"] == (cint, [i32, i32, i32, vp, vp, vp])
    assert h.signatures["ts_ctc_beam_piece_lm_workspace_bytes"] == (i64, [i32, i32, i32, i32])
    assert h.signatures["ts_ctc_beam_piece_lm_search"] == (cint, [vp, i32, i32, i32, i32, vp, i32, i32, i32, i32, i32, lm, lexicon, pieces] + [vp] * 8)
    assert (h.version_define, h.version_function, h.abi_version) == ("TS_CTC_BEAM_PIECE_LM_ABI_VERSION", "ts_ctc_beam_piece_lm_abi_version", 1)
    assert list(h.structs) == ["ts_ctc_pieces"] and h.structs["ts_ctc_pieces"] is _lib.CtcPieces and _lib.CtcPieces._fields_ == FIELDS
    assert h.defines == {"TS_CTC_BEAM_PIECE_LM_ABI_VERSION": 1}
    # the search takes the word-level search's arguments plus the pieces; the sibling header is as it was
    word = _lib.OPEN["ctc_beam_word_lm"]
    assert [a for a in h.signatures["ts_ctc_beam_piece_lm_search"][1] if a is not pieces] == word.signatures["ts_ctc_beam_word_lm_search"][1]
    assert word.abi_version == 1 and list(word.structs) == ["ts_ctc_lexicon"] and list(_lib.OPEN) == sorted(_lib.OPEN)
    others = [_lib.CORE, *_lib.COMPANIONS.values(), *_lib.STAGED.values(), *_lib.QUEUED.values(), *(o for k, o in _lib.OPEN.items() if k != "ctc_beam_piece_lm")]
    assert not set().union(*(o.signatures for o in others)) & set(NAMES)


def test_built_library_exports_the_names_and_reports_the_version():
    from thunder_speech_amd import _lib, build as b
    path = b.build(verbose=False)
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert not [n for n in NAMES if n not in defined]
    assert _lib.lib().ts_ctc_beam_piece_lm_abi_version() == _lib.OPEN["ctc_beam_piece_lm"].abi_version == 1
    assert _lib.OPEN["ctc_beam_piece_lm"].path in b.header_deps()


# ---- 2. from_arpa --------------------------------------------------------------------------------------------------------------------------------
def test_from_arpa_builds_letters_pieces_and_the_trie_of_the_fixture():
    lm, ch = _lm(), _char_lm()
    assert lm.itos == PIECES and lm.blank_idx == 0 and lm.n_classes == 15 and lm.word_start == "▁"
    assert lm.letters == ["a", "c", "e", "o", "s", "t"]
    assert lm.piece_kind == [0, 2, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0] and lm.unspellable_classes == [1]
    assert ["".join(lm.letters[i] for i in p) for p in lm.piece_letters] == ["", "", "", "a", "c", "ca", "cat", "s", "a", "c", "e", "o", "s", "t", "at"]
    # "dog" cannot be spelled: one word, three n-grams; everything else is WordNGramLM's over the same file
    assert lm.dropped == 1 and lm.dropped_ngrams == 3 and lm.order == 3
    assert lm.words == ch.words and lm.lm_words == ch.lm_words and lm.word_class == ch.word_class and lm.unk_class == ch.unk_class == 12
    assert lm.lm.grams == ch.lm.grams and lm.lm.arcs == ch.lm.arcs and lm.lm.backoff == ch.lm.backoff
    assert lm.n_nodes == ch.n_nodes == 27 and lm.node_word == ch.node_word
    # the same trie with letter ids where the character vocabulary has classes (letter id + 2 there)
    assert [[(c + 2, n) for c, n in e] for e in lm.edges] == ch.edges
    hot = _lm(hotwords=["tea", "cat", "dog"], lexicon=["cat", "a", "tea", "zebra", "ca▁t"])
    assert hot.words == ["a", "cat", "tea"] and hot.hot == [False, True, True] and hot.dropped == 3       # "dog", "zebra", "ca▁t"
    assert hot.word_class == [hot.lm_words.index("a"), hot.lm_words.index("cat"), hot.unk_class]
    up = type(lm).from_arpa(ARPA, [p.upper() for p in PIECES], 0, spell=str.upper)
    assert up.words == lm.words and up.score(_ids("▁ca", "t", "▁s", "at"), eos=True) == pytest.approx(lm.score(_ids("▁ca", "t", "▁s", "at"), eos=True))
    # word_start anywhere but at the front, and the specials, have no spelling; another word_start is honoured
    odd = type(lm).from_arpa(ARPA, ["a▁c", "<s>", "</s>", "▁▁", "_ca", "t", "<pad>"], 6, word_start="_")
    assert odd.piece_kind == [0, 2, 2, 0, 1, 0, 0] and odd.unspellable_classes == [1, 2] and odd.letters == ["a", "c", "t", "▁"]
    assert type(lm).from_arpa(ARPA, ["a▁c", "▁▁", "▁ca", "t", "<pad>"], 4).piece_kind == [2, 2, 1, 0, 0]
    with pytest.raises(ValueError, match="not hot words"):
        _lm(hotwords=["cot"]).weights(0.5, 1.0, boosts={"cat": 1.0}, device="cpu")


def test_word_ngram_lm_still_refuses_this_vocabulary():
    from thunder_speech_amd.ctc_lm import WordNGramLM
    with pytest.raises(ValueError, match="no class ' ' to end a word"):
        WordNGramLM.from_arpa(ARPA, PIECES, 0)


# ---- 3. the host walk ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("word,n_seg", [("cat", 6), ("cats", 6), ("seat", 4)])
def test_every_segmentation_of_a_word_reaches_the_same_node_and_the_same_score(word, n_seg):
    lm = _lm()
    segs = _segmentations(word)
    assert len(segs) == n_seg and all("".join(s).replace("▁", "") == word for s in segs)
    ends, scores = set(), set()
    for seg in segs:
        s, x = lm.start_state, 0
        for c in _ids(*seg):
            r = lm.step(s, x, c)
            assert r.log10 == 0.0 and r.oov == 0 and r.word is None and r.state == s
            s, x = r.state, r.x
        ends.add(x)
        scores |= {(lm.score(_ids(*seg), eos), lm.score(_ids("▁a", *seg), eos)) for eos in (False, True)}
    assert len(ends) == 1 and lm.words[lm.node_word[ends.pop()]] == word and len(scores) == 2


def test_walk_over_pieces_equals_the_character_walk_over_the_same_text():
    """Random texts -- words of the lexicon and random spellings, now and then an empty word (a bare word start before the next word) --, cut into
    pieces at random: (log10, OOV count, words) are those of WordNGramLM.walk over the text's characters, with and without </s>; the lexicon leaves
    out some of the LM's words and holds hot words that the LM lacks."""
    kw = dict(lexicon=["a", "at", "cat", "cot", "eat", "oat", "sat", "set", "tea", "ace", "seat"], hotwords=["cot", "tea"], unk_log10=-6.25)
    lm, ch = _lm(**kw), _char_lm(**kw)
    assert lm.words == ch.words and lm.hot == ch.hot
    rng = np.random.Generator(np.random.PCG64(11))
    met = set()
    for _ in range(400):
        words = [lm.words[int(rng.integers(len(lm.words)))] if rng.random() < 0.6 else "".join(rng.choice(list("aceost"), int(rng.integers(1, 5))))
                 for _ in range(int(rng.integers(0, 5)))]
        pieces, text = [], ""
        for w in words:
            if rng.random() < 0.15:
                pieces.append("▁")                                           # an empty word: a doubled delimiter in the character text
                text += " "
            seg = _segmentations(w)
            pieces += seg[int(rng.integers(len(seg)))]
            text += " " + w
        for eos in (False, True):
            got, want = lm.walk(_ids(*pieces), eos), ch.walk([CHARS.index(c) for c in text], eos)
            assert got[0] == pytest.approx(want[0], abs=1e-12) and got[1:] == want[1:], (pieces, text)
        met |= {"oov"} if got[1] else set()
        met |= {"hot"} if any(lm.hot[w] for w in got[2]) else set()
        met |= {"unk-in-lexicon"} if any(lm.word_class[w] == lm.unk_class for w in got[2]) else set()
    assert met == {"oov", "hot", "unk-in-lexicon"}


def test_where_the_oov_factor_is_paid():
    lm = _lm(lexicon=["cot", "a", "cat"])
    s0 = lm.start_state
    # a piece that leaves the trie in its second letter pays once, and the rest of the word pays nothing
    small = _lm(lexicon=["cot", "a"])
    r = small.step(s0, 0, PIECES.index("▁ca"))
    assert (r.x, r.oov, r.log10, r.state, r.word) == (-1, 1, 0.0, s0, None)
    assert small.step(s0, -1, PIECES.index("at")) == (0.0, s0, -1, 0, None)
    assert small.walk(_ids("▁ca", "t"))[1:] == (1, []) and small.walk(_ids("▁ca", "at", "s", "▁a"))[1:] == (1, [small.words.index("a")])
    # <unk> inside a word makes the word OOV, once; outside the lexicon already it changes nothing; it never ends a word
    x_c = lm.step(s0, 0, PIECES.index("▁c")).x
    assert x_c > 0 and lm.step(s0, x_c, 1) == (0.0, s0, -1, 1, None) and lm.step(s0, -1, 1) == (0.0, s0, -1, 0, None)
    assert lm.step(s0, 0, 1) == (0.0, s0, -1, 1, None)                        # at the root too: <unk> is a word of one unknown letter
    assert lm.walk(_ids("▁c", "<unk>", "a", "t"))[1:] == (1, []) and lm.walk(_ids("▁c", "<unk>", "<unk>", "▁cat"))[1:] == (1, [lm.words.index("cat")])
    # a piece that ends a word at a node that is no word and leaves the trie with its own letters pays twice: one factor per word
    r = lm.step(s0, x_c, PIECES.index("▁s"))
    assert (r.x, r.oov, r.word) == (-1, 2, None) and r.log10 == pytest.approx(lm.lm.step(s0, lm.unk_class)[0])
    assert lm.walk(_ids("▁c", "▁s"))[1] == 2 and lm.walk(_ids("▁c", "e", "▁s", "e", "▁cat"))[1:] == (2, [lm.words.index("cat")])
    with pytest.raises(ValueError, match="is the blank"):
        lm.step(s0, 0, 0)
    with pytest.raises(ValueError, match="outside the classes"):
        lm.step(s0, 0, len(PIECES))


def test_a_bare_word_start_ends_a_word_and_two_in_a_row_end_none():
    lm = _lm()
    s0 = lm.start_state
    assert lm.step(s0, 0, 2) == (0.0, s0, 0, 0, None)                         # at the start of a clip: nothing
    x = lm.walk(_ids("▁cat"))                                                 # (the pending word counts in walk)
    s, xc = s0, 0
    for c in _ids("▁ca", "t"):
        s, xc = lm.step(s, xc, c)[1:3]
    r = lm.step(s, xc, 2)
    assert r.word == lm.words.index("cat") and r.x == 0 and r.oov == 0 and r.log10 == pytest.approx(-0.7) and r.state != s0
    assert lm.step(r.state, 0, 2) == (0.0, r.state, 0, 0, None)               # the second one in a row
    assert lm.walk(_ids("▁ca", "t", "▁", "▁")) == lm.walk(_ids("▁ca", "t", "▁")) == x
    # continuation pieces after a bare word start spell the next word
    assert lm.walk(_ids("▁", "c", "at", "▁", "s", "a", "t"), True) == lm.walk(_ids("▁cat", "▁s", "at"), True)
    assert lm.walk(_ids("▁cat", "▁s", "at"), True)[0] == pytest.approx(-0.7 + (-0.1 - 0.6) + (-0.15 - 0.2 - 1.1))    # <s> cat; bo(<s> cat), cat sat; </s> by two back-offs


# ---- 4. the tables -------------------------------------------------------------------------------------------------------------------------------
def test_piece_and_lexicon_tables_are_well_formed():
    lm = _lm(hotwords=["cot", "tea"])
    p = lm.piece_tables()
    assert {k: (v.dtype, v.shape) for k, v in p.items()} == {"piece_begin": (np.int32, (16,)), "piece_letter": (np.int32, (16,)), "piece_kind": (np.int32, (15,))}
    assert p["piece_begin"][0] == 0 and p["piece_begin"][-1] == len(p["piece_letter"]) and (np.diff(p["piece_begin"]) >= 0).all()
    assert p["piece_letter"].min() >= 0 and p["piece_letter"].max() < len(lm.letters)
    for c, tok in enumerate(PIECES):
        spelt = "".join(lm.letters[i] for i in p["piece_letter"][p["piece_begin"][c]: p["piece_begin"][c + 1]])
        assert spelt == ("" if c < 2 else tok.lstrip("▁")) and p["piece_kind"][c] == (2 if tok == "<unk>" else int(tok.startswith("▁")))
    t = lm.lexicon_tables(oov_score=-3.0, hotword_weight=1.5, boosts={"tea": 4.0})
    n = lm.n_nodes
    assert t["edge_begin"].shape == (n + 1,) and t["edge_begin"][0] == 0 and t["edge_begin"][-1] == n - 1 == len(t["edge_class"]) == len(t["edge_next"])
    for x in range(n):
        cls = t["edge_class"][t["edge_begin"][x]: t["edge_begin"][x + 1]].tolist()
        assert cls == sorted(set(cls)) and all(0 <= c < len(lm.letters) for c in cls)                  # sorted by letter, no letter twice
    assert ((t["edge_next"] > 0) & (t["edge_next"] < n)).all() and t["node_word"].tolist() == lm.node_word
    np.testing.assert_array_equal(t["word_factor"], np.exp(np.array([4.0 if w == "tea" else 1.5 if w == "cot" else 0.0 for w in lm.words])))
    assert t["oov_factor"].tolist() == [np.exp(-3.0)]


# ---- 5. the launcher -----------------------------------------------------------------------------------------------------------------------------
def _structs(lm_over, lx_over, pc_over):
    from thunder_speech_amd import _lib
    A = 0x20000
    lm = dict(n_states=3, n_arcs=7, start_state=1, has_eos=1, arc_begin=A, arc_class=A, arc_next=A, arc_factor=A, arc_log10=A, bo_next=A, bo_factor=A,
              bo_log10=A, eos_factor=A, eos_log10=A)
    lx = dict(n_nodes=5, n_edges=4, n_words=2, delimiter=-1, unk_class=2, edge_begin=A, edge_class=A, edge_next=A, node_word=A, word_class=A,
              word_factor=A, oov_factor=A)
    pc = dict(n_classes=8, n_letters=6, n_piece_letters=9, piece_begin=A, piece_letter=A, piece_kind=A)
    lm.update(lm_over)
    lx.update(lx_over)
    pc.update(pc_over)
    return _lib.CtcLm(**lm), _lib.CtcLexicon(**lx), _lib.CtcPieces(**pc)


def _host_cases():
    """(arguments of ts_ctc_beam_piece_lm_search, expected status) of calls that return before any launch.  Pointers are made-up addresses (never
    dereferenced on these paths).  `lm` / `lx` / `pc`: fields of the three structs to override, or None for a NULL struct."""
    A, E, U = 0x10000, -1, -2
    bs = lambda lg=A, b=2, v=8, t=50, pitch=64, il=A, blank=0, w=16, cap=4, nb=2, eos=1, lm={}, lx={}, pc={}, tok=A, fr=A, ln=A, sc=A, lsc=A, cnt=A, ws=A: (
        lg, b, v, t, pitch, il, blank, w, cap, nb, eos, lm, lx, pc, tok, fr, ln, sc, lsc, cnt, ws, None)
    return [
        (bs(lg=0), E), (bs(tok=0), E), (bs(fr=0), E), (bs(ln=0), E), (bs(sc=0), E), (bs(lsc=0), E), (bs(cnt=0), E), (bs(ws=0), E), (bs(lm=None), E),
        (bs(lx=None), E), (bs(pc=None), E),
        (bs(b=0), E), (bs(v=0), E), (bs(t=0), E), (bs(pitch=49), E), (bs(blank=-1), E), (bs(blank=8, pc=dict(n_classes=8)), E),
        (bs(w=0), E), (bs(cap=0), E), (bs(nb=0), E), (bs(nb=17), E), (bs(w=1, nb=2), E),
        (bs(w=65), U), (bs(cap=65), U), (bs(w=64, nb=65, v=4, pc=dict(n_classes=4)), U), (bs(ws=A + 8), U),
        (bs(v=(1 << 24) + 1, pc=dict(n_classes=(1 << 24) + 1)), U),
        # the 1024-candidate limit: beam_width (min(token_cap, n_classes - 1) + 1)
        (bs(v=32, w=64, cap=16, pc=dict(n_classes=32)), U), (bs(v=1025, w=33, cap=31, pc=dict(n_classes=1025)), U),
        # the word automaton and the lexicon, as in the sibling
        (bs(lm=dict(arc_begin=0)), E), (bs(lm=dict(eos_log10=0)), E), (bs(lm=dict(n_states=0)), E), (bs(lm=dict(start_state=3)), E),
        (bs(lm=dict(arc_factor=0x20004)), U),
        (bs(lx=dict(edge_begin=0)), E), (bs(lx=dict(edge_class=0)), E), (bs(lx=dict(edge_next=0)), E), (bs(lx=dict(node_word=0)), E),
        (bs(lx=dict(word_class=0)), E), (bs(lx=dict(word_factor=0)), E), (bs(lx=dict(oov_factor=0)), E), (bs(lx=dict(n_nodes=0)), E),
        (bs(lx=dict(n_edges=-1)), E), (bs(lx=dict(n_words=-1)), E), (bs(lx=dict(oov_factor=0x20004)), U),
        # the delimiter is not looked at: whatever it holds, the call goes on to the next refusal (the misaligned workspace)
        (bs(lx=dict(delimiter=-1), ws=A + 8), U), (bs(lx=dict(delimiter=0), ws=A + 8), U), (bs(lx=dict(delimiter=99), ws=A + 8), U),
        # the pieces
        (bs(pc=dict(piece_begin=0)), E), (bs(pc=dict(piece_letter=0)), E), (bs(pc=dict(piece_kind=0)), E), (bs(pc=dict(n_classes=7)), E),
        (bs(pc=dict(n_classes=9)), E), (bs(pc=dict(n_letters=-1)), E), (bs(pc=dict(n_piece_letters=-1)), E),
        (bs(pc=dict(piece_letter=0, n_piece_letters=0), ws=A + 8), U),       # no letters at all: no table needed
    ]


@pytest.mark.parametrize("args,want", _host_cases())
def test_launcher_refuses_bad_arguments_before_any_launch(args, want):
    from thunder_speech_amd import _lib
    assert (_lib.TS_EINVAL, _lib.TS_EUNSUPPORTED) == (-1, -2)
    lm, lx, pc = args[11:14]
    keep = _structs(lm or {}, lx or {}, pc or {})
    refs = tuple(None if given is None else ctypes.byref(k) for given, k in zip((lm, lx, pc), keep))
    assert _lib.lib().ts_ctc_beam_piece_lm_search(*args[:11], *refs, *args[14:]) == want


def _query(L, n_classes, width, cap):
    out = [ctypes.c_int32(-7) for _ in range(3)]
    st = L.ts_ctc_beam_piece_lm_launch_config(n_classes, width, cap, *[ctypes.addressof(o) for o in out])
    return st, tuple(o.value for o in out)


def _expected(n_classes, width, cap):
    """The header's formulas: threads, LDS bytes, candidates."""
    cap = min(cap, n_classes - 1)
    cands = width * (cap + 1)
    up = lambda x, m: (x + m - 1) // m * m
    return up(cands, 64), 96 * up(width, 8) + 16 * up(cands, 8) + 48 * up(cap + 2, 2) + 2064, cands


@pytest.mark.parametrize("n_classes,width,cap", [(1025, 16, 8), (1025, 64, 15), (1025, 32, 31), (1025, 1, 1), (3, 64, 2), (2, 1, 1), (1, 4, 4), (129, 1, 64),
                                                 (15, 7, 3), (70, 16, 8), (16, 64, 64), (1 << 24, 15, 64)])
def test_launch_config_follows_the_header_formulas(n_classes, width, cap):
    from thunder_speech_amd import _lib
    L = _lib.lib()
    st, got = _query(L, n_classes, width, cap)
    assert st == 0 and got == _expected(n_classes, width, cap)
    threads, lds, cands = got
    assert cands <= threads <= 1024 and lds <= 28 * 1024
    out = [ctypes.c_int32(-7) for _ in range(3)]                             # the sibling's values
    assert L.ts_ctc_beam_word_lm_launch_config(n_classes, width, cap, *[ctypes.addressof(o) for o in out]) == 0 and tuple(o.value for o in out) == got


def test_launch_config_refusals_and_the_workspace_formula():
    from thunder_speech_amd import _lib
    L = _lib.lib()
    assert _query(L, 1025, 64, 15) == (0, (1024, 96 * 64 + 16 * 1024 + 48 * 18 + 2064, 1024))     # the largest workgroup there is
    for bad, want in (((0, 16, 8), -1), ((1025, 0, 8), -1), ((1025, 16, 0), -1), ((1025, 65, 8), -2), ((1025, 16, 65), -2), (((1 << 24) + 1, 16, 8), -2),
                      ((1025, 64, 16), -2), ((17, 61, 16), -2), ((1025, 33, 31), -2), ((1025, 64, 64), -2)):
        assert _query(L, *bad)[0] == want
    assert _query(L, 16, 64, 16)[0] == 0                                      # the clamped cap counts: 64 (15 + 1)
    out = ctypes.c_int32(0)
    assert L.ts_ctc_beam_piece_lm_launch_config(1025, 16, 8, None, ctypes.addressof(out), ctypes.addressof(out)) == -1
    f = lambda b, t, w, cap: b * (32 * (t * w + 1) + 12 * t * (cap + 2) + 512 * t + 768)
    for args in ((1, 1, 1, 1), (16, 250, 16, 8), (64, 188, 64, 15), (64, 751, 64, 64), (3, 37, 7, 3)):
        assert L.ts_ctc_beam_piece_lm_workspace_bytes(*args) == f(*args) == L.ts_ctc_beam_word_lm_workspace_bytes(*args)
    assert L.ts_ctc_beam_piece_lm_workspace_bytes(70000, 70000, 64, 64) == f(70000, 70000, 64, 64) > 2 ** 32    # 64-bit arithmetic
    for bad, want in (((0, 50, 16, 4), -1), ((2, 0, 16, 4), -1), ((2, 50, 0, 4), -1), ((2, 50, 16, 0), -1), ((2, 50, 65, 4), -2), ((2, 50, 16, 65), -2)):
        assert L.ts_ctc_beam_piece_lm_workspace_bytes(*bad) == want


# ---- 6. the module -------------------------------------------------------------------------------------------------------------------------------
def _tiny_citrinet():
    """The random tiny Citrinet of citrinet/compatibility.py with the test's pieces as its vocabulary (the blank comes last there)."""
    from thunder_speech_amd.citrinet.compatibility import build_synthetic_citrinet
    from thunder_speech_amd.text_processing.transform import BatchTextTransformer
    torch.manual_seed(0)
    module = build_synthetic_citrinet(filters=[64] * 5, kernel_sizes=[11, 13, 15, 17, 19], strides=[2, 1, 2, 1, 2], n_tokens=len(PIECES) - 1)
    module.text_transform = BatchTextTransformer(tokens=PIECES[1:])
    assert module.text_transform.vocab.itos == PIECES[1:] + ["<blank>"] and module.text_transform.num_tokens == len(PIECES)
    return module


def test_the_module_refuses_an_lm_of_another_vocabulary_and_cpu_tensors():
    from thunder_speech_amd.ctc_lm import NGramLM, PieceWordNGramLM, beam_search_piece_lm
    module = _tiny_citrinet()
    vocab = module.text_transform.vocab
    x = torch.zeros(1, 8000)
    other = vocab.itos[:5] + ["▁co"] + vocab.itos[6:]
    for lm, what in ((PieceWordNGramLM.from_arpa(ARPA, other, vocab.blank_idx), r"class 5 is '▁co' there and '▁cat' in this module"),
                     (PieceWordNGramLM.from_arpa(ARPA, vocab.itos + ["x"], vocab.blank_idx), r"class 15 is 'x' there and no such class in this module"),
                     (_lm(), "blank at class 0, this module's blank is class 14")):
        with pytest.raises(ValueError, match=what):
            module.predict_beam(x, lm=lm)
        with pytest.raises(ValueError, match=what):
            module.predict_nbest(x, 2, lm=lm)
        with pytest.raises(ValueError, match=what):
            module.transcribe_long([x[0]], beam_width=4, lm=lm)
    lm = PieceWordNGramLM.from_arpa(ARPA, vocab.itos, vocab.blank_idx, hotwords=["cot"])
    with pytest.raises(RuntimeError, match=r"GPU tensors required \(no CPU fallback\)"):
        module.predict_beam(x, lm=lm, hotword_weight=2.0, oov_score=-3.0, boosts={"cot": 1.0})
    with pytest.raises(RuntimeError, match=r"beam_search_piece_lm: GPU tensors required \(no CPU fallback\)"):
        beam_search_piece_lm(torch.zeros(1, 15, 9), lm, 0.5, 1.0, blank_idx=14)
    with pytest.raises(RuntimeError, match=r"PieceWordNGramLM.weights: GPU tensors required \(no CPU fallback\)"):
        lm.weights(0.5, 1.0, device="cpu")
    # the lexicon keywords still need an LM with a lexicon
    token_lm = NGramLM.from_arpa(os.path.join(ROOT, "tests", "golden", "lm_tiny.arpa"), vocab.itos, vocab.blank_idx)
    for given in (token_lm, None):
        with pytest.raises(ValueError, match="PieceWordNGramLM"):
            module.predict_beam(x, lm=given, oov_score=-3.0)
