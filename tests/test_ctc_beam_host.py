"""CTC prefix beam search on the CPU (the companion C header: tests/test_abi_headers_host.py): that the older CTC sources are left alone,
the argument checks of the launcher (made-up pointers: none of these calls reaches a launch), the launch-config and workspace formulas at the
limits, the refusal of CPU tensors, and the host-side conversion from the device tables to Hypothesis lists."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_older_ctc_sources_are_not_touched_by_the_beam_search():
    src = open(os.path.join(ROOT, "thunder_speech_amd", "csrc", "ctc_beam.hip")).read()
    assert '#include "thunder_speech_amd/ctc_beam.h"' in src and not re.search(r'#include\s+"[^"]*\.hip"', src)
    for name in ("ctc.hip", "ctc_align.hip", "decode.hip"):
        assert "ts_ctc_beam" not in open(os.path.join(ROOT, "thunder_speech_amd", "csrc", name)).read()
    assert "atomic" not in re.sub(r"//[^\n]*", "", src)                       # equal arguments give equal bits


# ---- argument checks ---------------------------------------------------------------------------------------------------------------------------
def _host_cases():
    """(entry point, arguments, expected status) of calls that return before any launch.  Pointers are made-up addresses (never dereferenced on
    these paths): A is 16-byte aligned."""
    A, E, U = 0x10000, -1, -2
    bs = lambda lg=A, b=2, v=8, t=50, pitch=64, il=A, blank=0, w=16, cap=4, nb=2, tok=A, fr=A, ln=A, sc=A, cnt=A, ws=A: (
        "ts_ctc_beam_search", (lg, b, v, t, pitch, il, blank, w, cap, nb, tok, fr, ln, sc, cnt, ws, None))
    wb = lambda b=2, t=50, w=16, cap=4: ("ts_ctc_beam_workspace_bytes", (b, t, w, cap))
    cases = [
        (bs(lg=0), E), (bs(tok=0), E), (bs(fr=0), E), (bs(ln=0), E), (bs(sc=0), E), (bs(cnt=0), E), (bs(ws=0), E),
        (bs(b=0), E), (bs(b=-1), E), (bs(v=0), E), (bs(t=0), E), (bs(t=-1), E), (bs(pitch=49), E), (bs(blank=-1), E), (bs(blank=8), E),
        (bs(w=0), E), (bs(cap=0), E), (bs(nb=0), E), (bs(w=-1), E), (bs(cap=-1), E), (bs(nb=-1), E), (bs(nb=17), E), (bs(w=1, nb=2), E),
        (bs(w=65), U), (bs(cap=65), U), (bs(w=64, nb=65), U), (bs(w=65, nb=65), U), (bs(w=1000, cap=1000, nb=1), U),
        (bs(ws=A + 8), U), (bs(ws=A + 4), U), (bs(v=(1 << 24) + 1, pitch=64), U),
        (wb(b=0), E), (wb(t=0), E), (wb(w=0), E), (wb(cap=0), E), (wb(w=65), U), (wb(cap=65), U),
    ]
    return [(name, args, want) for (name, args), want in cases]


@pytest.mark.parametrize("name,args,want", _host_cases(), ids=lambda v: v if isinstance(v, str) else None)
def test_launcher_refuses_bad_arguments_before_any_launch(name, args, want):
    from thunder_speech_amd import _lib
    assert (_lib.TS_EINVAL, _lib.TS_EUNSUPPORTED) == (-1, -2)
    assert getattr(_lib.lib(), name)(*args) == want


# ---- the launch-config query and the workspace ------------------------------------------------------------------------------------------------
def _query(L, n_classes, width, cap):
    out = [ctypes.c_int32(-7) for _ in range(3)]
    st = L.ts_ctc_beam_launch_config(n_classes, width, cap, *[ctypes.addressof(o) for o in out])
    return st, tuple(o.value for o in out)


def _expected(n_classes, width, cap):
    """The header's formulas: ranked candidates, threads, LDS bytes."""
    cap = min(cap, n_classes - 1)
    cands = width + cap + sum(min(cap, -(-width // i)) for i in range(1, width))
    up = lambda x, m: (x + m - 1) // m * m
    return up(cands, 64), 88 * up(width, 8) + 16 * up(cands, 8) + 48 * up(cap + 2, 2) + 2064, cands


@pytest.mark.parametrize("n_classes,width,cap", [(29, 16, 8), (32, 64, 16), (1025, 64, 64), (1025, 1, 1), (3, 64, 2), (2, 1, 1), (1, 4, 4), (29, 1, 64),
                                                 (5, 7, 3), (257, 32, 32), (29, 64, 64), (1 << 24, 64, 64)])
def test_launch_config_follows_the_header_formulas(n_classes, width, cap):
    from thunder_speech_amd import _lib
    st, got = _query(_lib.lib(), n_classes, width, cap)
    assert st == 0 and got == _expected(n_classes, width, cap)
    threads, lds, cands = got
    assert width <= cands <= width * (min(cap, n_classes - 1) + 1) and threads <= 512 and lds <= 20 * 1024


def test_launch_config_at_the_limits_and_its_refusals():
    from thunder_speech_amd import _lib
    L = _lib.lib()
    assert L.ts_ctc_beam_abi_version() == 1
    assert _query(L, 1025, 64, 64) == (0, (512, 88 * 64 + 16 * 464 + 48 * 66 + 2064, 464))     # the largest workgroup there is
    assert _query(L, 29, 16, 8)[1][0] == 128 and _query(L, 29, 64, 16)[1][0] == 384
    assert _query(L, 29, 4, 2)[1][2] == 4 * 3                                # narrow beams rank every child: ceil(W / i) >= cap for every slot
    for bad, want in (((0, 16, 8), -1), ((29, 0, 8), -1), ((29, 16, 0), -1), ((29, 65, 8), -2), ((29, 16, 65), -2), (((1 << 24) + 1, 16, 8), -2)):
        assert _query(L, *bad)[0] == want
    out = ctypes.c_int32(0)
    assert L.ts_ctc_beam_launch_config(29, 16, 8, None, ctypes.addressof(out), ctypes.addressof(out)) == -1


def test_workspace_formula():
    from thunder_speech_amd import _lib
    L = _lib.lib()
    f = lambda b, t, w, cap: b * (16 * (t * w + 1) + 12 * t * (cap + 2) + 512 * t + 256)
    for args in ((1, 1, 1, 1), (16, 999, 16, 8), (16, 999, 64, 16), (64, 751, 64, 64), (3, 37, 7, 3)):
        assert L.ts_ctc_beam_workspace_bytes(*args) == f(*args)
    assert L.ts_ctc_beam_workspace_bytes(70000, 70000, 64, 64) == f(70000, 70000, 64, 64) > 2 ** 32        # 64-bit arithmetic


# ---- no CPU path -------------------------------------------------------------------------------------------------------------------------------
def test_cpu_tensors_are_refused():
    from thunder_speech_amd.ctc_beam import beam_search
    from thunder_speech_amd.registry import load_pretrained
    module = load_pretrained("QuartzNet5x5_synthetic")
    x = torch.zeros(1, 4000)
    with pytest.raises(RuntimeError, match=r"GPU tensors required \(no CPU fallback\)"):
        module.predict_beam(x)
    with pytest.raises(RuntimeError, match=r"GPU tensors required \(no CPU fallback\)"):
        module.predict_nbest(x, 3)
    with pytest.raises(RuntimeError, match=r"beam_search: GPU tensors required \(no CPU fallback\)"):
        beam_search(torch.zeros(1, 5, 9))


# ---- device tables -> hypotheses ---------------------------------------------------------------------------------------------------------------
def test_hypotheses_from_hand_made_tables():
    from thunder_speech_amd.ctc_beam import BeamToken, Hypothesis, hypotheses_from_tables
    itos = ["<blank>", "h", "i", "|", "o"]
    to_text = lambda ids: "".join(itos[i] for i in ids).replace("|", " ")
    tokens = np.zeros((2, 3, 6), np.int32)
    frames = np.zeros((2, 3, 6), np.int32)
    tokens[0, 0, :4], frames[0, 0, :4] = [1, 2, 3, 4], [0, 2, 3, 5]
    tokens[0, 1, :2], frames[0, 1, :2] = [1, 2], [0, 2]
    tokens[0, 2, :3] = [4, 4, 4]                                             # beyond the count: must not appear
    lengths = np.array([[4, 2, 3], [0, 0, 0]], np.int32)
    scores = np.array([[-0.5, -1.25, -9.0], [0.0, -np.inf, -np.inf]], np.float32)
    counts = np.array([2, 1], np.int32)
    got = hypotheses_from_tables(tokens, frames, lengths, scores, counts, itos, to_text, 320, 16000)
    assert [len(c) for c in got] == [2, 1]
    assert got[0][0] == Hypothesis("hi o", -0.5, [BeamToken("h", 0, 0.0), BeamToken("i", 2, 0.04), BeamToken("|", 3, 0.06), BeamToken("o", 5, 0.1)])
    assert got[0][1] == Hypothesis("hi", -1.25, [BeamToken("h", 0, 0.0), BeamToken("i", 2, 0.04)])
    assert got[1][0] == Hypothesis("", 0.0, [])                              # the empty transcript is a hypothesis
    assert all(isinstance(t.frame, int) and isinstance(t.time, float) for t in got[0][0].tokens)
    assert hypotheses_from_tables(tokens, frames, lengths, scores, np.zeros(2, np.int32), itos, to_text, 320, 16000) == [[], []]
