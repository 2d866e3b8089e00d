"""ts_ctc_align and ts_ctc_greedy_spans (csrc/ctc_align.hip, include/thunder_speech_amd/ctc_align.h) against float64 on the CPU, through the raw
ABI, and BaseCTCModule.align / predict_spans through two model families.

The reference is `_viterbi64` below: the Viterbi recursion over the blank-extended target on log_softmax in float64, a Python loop over the frames
with the states of a frame side by side in numpy, and the tie rule of the ABI (stay beats s-1, s-1 beats s-2, the path ends in the last label
state unless the final blank is strictly better).  `_viterbi64_loops` is the same thing as a plain double loop; the two are compared once
(in the first equality case).
Nothing of the package takes part in either.

Every case: the kernel's path has length T, collapses to the target and is -1 beyond T; its score recomputed in float64 along that path is within
the tolerance of the optimum; the `score` output agrees with the optimum within  2 T 2^-24  relative (the worst case of an f32 sum of T same-sign
terms, each rounded once from f64, with room for the normaliser); spans are the run boundaries of the kernel's own path and span_logp the float64
sums within the same bound.  Ratios error / bound are printed as `RATIO|kind|ratio|case` (profiles/ctc_align.md records them).

Exact path equality is demanded where the test itself asserts the margin condition in float64: the smallest gap between the best and the
second-best candidate at the cells of the optimal path, and at the final state, exceeds  E = 3 T 2^-24 M,  M the largest magnitude of any
partial path sum in the log-probability or the raw-logit formulation (the kernel's recursion runs on raw logits).  Under it no f32 rounding of
the partial sums can flip a decision on the path.  The seeds were picked on the CPU; the assertion of the condition stays in the test."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

U = 2.0 ** -24
NEG = -np.inf


# ---- the float64 reference -----------------------------------------------------------------------------------------------------------------------
def _ext(target, blank):
    ext = np.full(2 * len(target) + 1, blank, dtype=np.int64)
    ext[1::2] = target
    return ext


def _viterbi64(emit, target, blank, want_margin=False):
    """emit [V, T] float64 (log-probabilities, or raw logits: the decisions are the same).  -> dict(score, states [T] or None, margin, big).
    margin: smallest (best - second best) over the cells of the returned path and the final choice; big: largest finite |partial sum|."""
    T, ext = emit.shape[1], _ext(target, blank)
    L = len(ext)
    if T == 0:
        return dict(score=0.0 if L == 1 else NEG, states=np.zeros(0, np.int64) if L == 1 else None, margin=np.inf, big=0.0)
    skip = np.zeros(L, bool)
    skip[3::2] = ext[3::2] != ext[1:-2:2]
    a = np.full(L, NEG)
    a[:2] = emit[ext[:2], 0]
    bp = np.zeros((T, L), np.int8)
    gaps = np.full((T, L), np.inf) if want_margin else None
    big = float(np.abs(a[np.isfinite(a)]).max(initial=0.0))
    for t in range(1, T):
        c1 = np.concatenate([[NEG], a])[:L]
        c2 = np.where(skip, np.concatenate([[NEG, NEG], a])[:L], NEG)
        best, k = a.copy(), np.zeros(L, np.int8)
        m = c1 > best
        best[m], k[m] = c1[m], 1
        m = c2 > best
        best[m], k[m] = c2[m], 2
        if want_margin:
            srt = np.sort(np.stack([a, c1, c2]), axis=0)
            with np.errstate(invalid="ignore"):
                g = srt[2] - srt[1]
            gaps[t] = np.where(np.isnan(g), np.inf, g)
        a = best + emit[ext, t]
        bp[t] = k
        big = max(big, float(np.abs(a[np.isfinite(a)]).max(initial=0.0)))
    s = L - 1 if (L == 1 or a[L - 1] > a[L - 2]) else L - 2
    if a[s] == NEG:
        return dict(score=NEG, states=None, margin=np.inf, big=big)
    margin = abs(a[L - 1] - a[L - 2]) if L > 1 else np.inf
    score, states = float(a[s]), np.zeros(T, np.int64)
    for t in range(T - 1, -1, -1):
        states[t] = s
        if want_margin:
            margin = min(margin, gaps[t, s])
        s -= int(bp[t, s])
    return dict(score=score, states=states, margin=float(margin), big=big)


def _viterbi64_loops(emit, target, blank):
    """The same recursion as a plain double loop -> (score, states)."""
    T, ext = emit.shape[1], _ext(target, blank)
    L = len(ext)
    a = [NEG] * L
    a[0] = emit[ext[0], 0]
    if L > 1:
        a[1] = emit[ext[1], 0]
    bp = [[0] * L for _ in range(T)]
    for t in range(1, T):
        new = [NEG] * L
        for s in range(L):
            best, k = a[s], 0
            if s >= 1 and a[s - 1] > best:
                best, k = a[s - 1], 1
            if s >= 2 and s % 2 == 1 and ext[s] != ext[s - 2] and a[s - 2] > best:
                best, k = a[s - 2], 2
            new[s], bp[t][s] = best + emit[ext[s], t], k
        a = new
    s = L - 1 if (L == 1 or a[L - 1] > a[L - 2]) else L - 2
    score, states = a[s], [0] * T
    for t in range(T - 1, -1, -1):
        states[t] = s
        s -= bp[t][s]
    return float(score), np.array(states)


def _the_two_statements_of_the_reference_agree():
    g = torch.Generator().manual_seed(5)
    emit = torch.log_softmax(2 * torch.randn(6, 41, generator=g, dtype=torch.float64), 0).numpy()
    for target in ([1, 2, 2, 3, 1, 1, 5, 4], [], [3]):
        want = _viterbi64_loops(emit, target, 0)
        got = _viterbi64(emit, target, 0)
        assert got["score"] == want[0] and np.array_equal(got["states"], want[1])
    zero = np.zeros((4, 9))
    assert np.array_equal(_viterbi64(zero, [1, 1, 2, 3], 0)["states"], _viterbi64_loops(zero, [1, 1, 2, 3], 0)[1])


# ---- cases through the raw ABI -------------------------------------------------------------------------------------------------------------------
def _target(g, s, v, blank, repeats):
    labels = [i for i in range(v) if i != blank]
    out = []
    for _ in range(s):
        pool = labels if repeats or not out else [x for x in labels if x != out[-1]]
        out.append(pool[int(torch.randint(len(pool), (1,), generator=g))])
    return out


def _case(name, v, blank, n_frames, s_max, utts, seed, pitch=None, zero=False, expect=None, equal=False):
    """utts: (input_len, target_len, repeats allowed) per utterance, or (input_len, explicit target list)."""
    return dict(name=name, v=v, blank=blank, n_frames=n_frames, s_max=s_max, utts=utts, seed=seed, pitch=pitch or n_frames + 5, zero=zero,
                expect=expect, equal=equal)


def _build(case):
    g = torch.Generator().manual_seed(case["seed"])
    b, v, n, pitch = len(case["utts"]), case["v"], case["n_frames"], case["pitch"]
    logits = torch.full((b, v, pitch), float("nan"))
    targets = torch.zeros(b, max(case["s_max"], 1), dtype=torch.int32)
    t_in, s_in = [], []
    for i, u in enumerate(case["utts"]):
        t = max(0, min(u[0], n))
        tg = list(u[1]) if isinstance(u[1], (list, tuple)) else _target(g, u[1], v, case["blank"], u[2])
        logits[i, :, :t] = 0.0 if case["zero"] else 2 * torch.randn(v, t, generator=g)       # NaN beyond input_len and in [n_frames, pitch)
        targets[i, : len(tg)] = torch.tensor(tg, dtype=torch.int32)
        t_in.append(u[0])
        s_in.append(len(tg))
    return logits, targets, torch.tensor(t_in, dtype=torch.int32), torch.tensor(s_in, dtype=torch.int32)


def _launch(case, logits, targets, t_in, s_in):
    from thunder_speech_amd import _lib
    L = _lib.lib()
    b, v, n, s_max = len(case["utts"]), case["v"], case["n_frames"], case["s_max"]
    dev = "cuda"
    lg = logits.to(dev)
    tg, il, tl = targets.to(dev), t_in.to(dev), s_in.to(dev)
    pad = 7                                                                                  # cells behind every output: nothing writes them
    path = torch.full((b * n + pad,), -77, dtype=torch.int32, device=dev)
    spans = torch.full((b * s_max * 2 + pad,), -77, dtype=torch.int32, device=dev)
    logp = torch.full((b * s_max + pad,), -77.0, device=dev)
    score = torch.full((b + pad,), -77.0, device=dev)
    ws = torch.full((int(L.ts_ctc_align_workspace_bytes(b, n, s_max)) + 16,), 0xFF, dtype=torch.uint8, device=dev)
    st = L.ts_ctc_align(lg.data_ptr(), b, v, n, case["pitch"], tg.data_ptr(), s_max, il.data_ptr(), tl.data_ptr(), case["blank"], path.data_ptr(),
                        spans.data_ptr(), logp.data_ptr(), score.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert st == 0, f"{case['name']}: ts_ctc_align returned {st}"
    torch.cuda.synchronize()
    assert torch.equal(lg.view(torch.int32).cpu(), logits.view(torch.int32)), "the logits were written"
    assert bool((ws[-16:] == 0xFF).all()), "bytes beyond the workspace were written"
    for buf in (path, spans, logp, score):
        assert bool((buf[-pad:] == -77).all()), f"{case['name']}: cells behind an output were written"
    return (path[:-pad].view(b, n).cpu().numpy(), spans[:-pad].view(b, s_max, 2).cpu().numpy(), logp[:-pad].view(b, s_max).cpu().numpy(),
            score[:-pad].cpu().numpy())


def _runs(row):
    """(id, first, end) of each run of equal ids."""
    out, t = [], 0
    while t < len(row):
        e = t + 1
        while e < len(row) and row[e] == row[t]:
            e += 1
        out.append((int(row[t]), t, e))
        t = e
    return out


def _check(case, got, logits, targets, t_in, s_in):
    """Optimality and validity of every utterance of a case; -> the reference results (for the equality checks of the callers)."""
    path, spans, logp, score = got
    n, s_max, blank = case["n_frames"], case["s_max"], case["blank"]
    refs = []
    for i in range(len(case["utts"])):
        T, S = max(0, min(int(t_in[i]), n)), max(0, min(int(s_in[i]), s_max))
        target = targets[i, :S].tolist()
        lp = torch.log_softmax(logits[i, :, :T].double(), 0).numpy()
        ref = _viterbi64(lp, target, blank, want_margin=case["equal"])
        refs.append(ref)
        what = f"{case['name']}[{i}] (T {T}, S {S})"
        if ref["states"] is None:                                     # infeasible
            assert score[i] == NEG and (path[i] == -1).all() and (spans[i] == 0).all() and (logp[i] == 0).all(), what
            continue
        assert np.isfinite(score[i]), f"{what}: score {score[i]} for a feasible utterance"
        assert (path[i, T:] == -1).all() and (path[i, :T] >= 0).all() and (path[i, :T] < case["v"]).all(), what
        runs = [r for r in _runs(path[i, :T]) if r[0] != blank]
        assert [r[0] for r in runs] == target, f"{what}: the path does not collapse to the target"
        tol = 2 * max(T, 1) * U
        along = float(lp[path[i, :T], np.arange(T)].sum())
        opt = ref["score"]
        print(f"RATIO|align-path|{(opt - along) / (tol * abs(opt)) if opt else 0.0:.3e}|{what} (optimum - score along the kernel's path) / (2 T u |optimum|)")
        print(f"RATIO|align-score|{abs(float(score[i]) - opt) / (tol * abs(opt)) if opt else abs(float(score[i])):.3e}|{what}")
        assert along >= opt - tol * abs(opt), f"{what}: the kernel's path scores {along}, the optimum is {opt}"
        assert abs(float(score[i]) - opt) <= tol * abs(opt), f"{what}: score {score[i]} against {opt}"
        assert (spans[i, S:] == 0).all() and (logp[i, S:] == 0).all(), what
        worst = 0.0
        for j, (_, f0, f1) in enumerate(runs):
            assert (int(spans[i, j, 0]), int(spans[i, j, 1])) == (f0, f1), f"{what}: span {j} is {spans[i, j]}, the path's run is {(f0, f1)}"
            want = float(lp[target[j], f0:f1].sum())
            worst = max(worst, abs(float(logp[i, j]) - want) / (tol * abs(want)))
        print(f"RATIO|align-span-logp|{worst:.3e}|{what}")
        assert worst <= 1.0, f"{what}: span_logp off by {worst:.3e} of the bound"
    return refs


def _run(case):
    built = _build(case)
    got = _launch(case, *built)
    return got, built, _check(case, got, *built)


def _path_of(states, target, blank):
    return _ext(target, blank)[states]


# ---- exact path equality under the margin condition ---------------------------------------------------------------------------------------------
# seeds: of the seeds 0 .. 11 every one meets the condition at T <= 60, seven at T = 200 and two (4, 7) at T = 300; these have the widest margin / E
EQUAL = [
    _case("eq-t41", 5, 0, 41, 20, [(41, 20, False)], seed=4, equal=True),
    _case("eq-t60", 8, 3, 60, 12, [(60, 12, True)], seed=7, equal=True),
    _case("eq-t200", 29, 28, 200, 40, [(200, 40, True)], seed=0, equal=True),
    _case("eq-t300", 6, 0, 300, 100, [(300, 100, True)], seed=4, equal=True),
]


def _margin_condition(case, built, refs):
    logits, targets, t_in, s_in = built
    out = []
    for i, ref in enumerate(refs):
        T, S = int(t_in[i]), int(s_in[i])
        raw = _viterbi64(logits[i, :, :T].double().numpy(), targets[i, :S].tolist(), case["blank"])
        assert np.array_equal(raw["states"], ref["states"])           # the normaliser shifts all paths alike: the same decisions in float64
        big = max(ref["big"], raw["big"])
        out.append((ref["margin"], 3 * T * U * big))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", EQUAL, ids=[c["name"] for c in EQUAL])
def test_path_equals_the_reference_where_the_margin_condition_holds(case):
    if case is EQUAL[0]:
        _the_two_statements_of_the_reference_agree()
    got, built, refs = _run(case)
    for i, (margin, e) in enumerate(_margin_condition(case, built, refs)):
        print(f"MARGIN|{case['name']}[{i}]|margin {margin:.3e}|E {e:.3e}")
        assert margin > e, f"{case['name']}: the fixture no longer meets the margin condition ({margin:.3e} <= {e:.3e}); pick another seed"
        T, S = int(built[2][i]), int(built[3][i])
        want = _path_of(refs[i]["states"], built[1][i, :S].tolist(), case["blank"])
        assert np.array_equal(got[0][i, :T], want), f"{case['name']}[{i}]: the path differs from the reference under the margin condition"


# ---- the tie rule --------------------------------------------------------------------------------------------------------------------------------
TIES = [
    _case("tie-t30-s7", 6, 0, 30, 7, [(30, [1, 2, 3, 4, 5, 1, 2])], seed=0, zero=True),
    _case("tie-t9-s4-exact", 6, 2, 9, 4, [(5, [1, 1, 3, 4]), (9, [1, 1, 3, 4])], seed=0, zero=True),         # T = S + repeats: exactly feasible
    _case("tie-s0", 4, 1, 12, 3, [(12, []), (1, [])], seed=0, zero=True),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", TIES, ids=[c["name"] for c in TIES])
def test_tie_rule_fixes_the_path_on_all_zero_logits(case):
    """Every candidate is bit-equal in f32 and in f64 (sums of equal log-probabilities in the reference, of zeros in the kernel), so the path
    is the rule's alone: stay, then s-1, then s-2; the last label state unless the final blank is strictly better."""
    got, built, refs = _run(case)
    for i, ref in enumerate(refs):
        T, S = int(built[2][i]), int(built[3][i])
        want = _path_of(ref["states"], built[1][i, :S].tolist(), case["blank"])
        assert np.array_equal(got[0][i, :T], want), f"{case['name']}[{i}]: {got[0][i, :T]} against {want}"


# ---- edges ---------------------------------------------------------------------------------------------------------------------------------------
EDGES = [
    _case("infeasible", 6, 0, 20, 8, [(5, [1, 1, 2, 3]), (0, [2, 3]), (20, [1, 1, 2, 3]), (4, [1, 2, 3, 4, 5]), (-3, [1])], seed=3),
    _case("empty-and-one-frame", 5, 4, 16, 4, [(16, []), (1, [2]), (1, []), (0, []), (1, [1, 2]), (2, [3, 3])], seed=4),
    _case("blank-first", 7, 0, 33, 9, [(33, 9, True), (31, 4, True)], seed=5),
    _case("blank-middle", 7, 3, 33, 9, [(33, 9, True), (20, 9, False)], seed=6),
    _case("blank-last", 7, 6, 33, 9, [(33, 9, True), (70, 5, True)], seed=7),                              # input_len beyond n_frames is clamped
    _case("wide-pitch", 9, 0, 65, 16, [(65, 16, True), (64, 16, True), (17, 3, False)], seed=8, pitch=192),  # target_len beyond s_max is clamped
    _case("s-max-zero", 5, 0, 10, 0, [(10, []), (0, [])], seed=9),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", EDGES, ids=[c["name"] for c in EDGES])
def test_edges(case):
    if case["name"] == "wide-pitch":
        built = list(_build(case))
        built[3] = built[3].clone()
        built[3][1] = 20                                              # 20 labels asked for, room for 16: the kernel reads 16
        got = _launch(case, *built)
        _check(case, got, *built)
    else:
        _run(case)


# ---- every instantiation, by name ---------------------------------------------------------------------------------------------------------------
INSTANCES = [
    # back-pointers in LDS: 1, 2 and 4 states per thread (the label capacity s_max picks the instantiation; n_frames must fit into 160 KiB)
    _case("lds-1-s40", 12, 0, 128, 40, [(128, 40, True), (90, 1, False)], seed=11, expect=(1, 128, 1)),
    _case("lds-1-s150-big", 32, 0, 999, 150, [(999, 150, True)], seed=12, expect=(1, 320, 1)),              # 80 KB of back-pointers: the opt-in beyond 64 KiB
    _case("lds-2-s600", 10, 4, 460, 600, [(460, 350, True), (459, 330, False)], seed=13, expect=(2, 640, 1)),
    _case("lds-4-s1030", 10, 9, 230, 1030, [(230, 150, True), (200, 200, False)], seed=14, expect=(4, 576, 1)),
    # back-pointers in the workspace: n_frames overflows LDS; the short input_len of the first row keeps its work small
    _case("ws-1-s40", 12, 5, 6000, 40, [(300, 40, True), (129, 17, True), (16, 16, False)], seed=15, expect=(1, 128, 0)),
    _case("ws-2-s600", 10, 0, 700, 600, [(700, 600, False), (650, 300, True)], seed=16, expect=(2, 640, 0)),
    _case("ws-4-s1030", 12, 0, 1300, 1030, [(1300, 1030, False), (1100, 513, True), (33, 2, True)], seed=17, expect=(4, 576, 0)),
]


def _query(L, n_frames, s_max):
    out = [C.c_int32(-7) for _ in range(4)]
    st = L.ts_ctc_align_launch_config(n_frames, s_max, *[C.addressof(o) for o in out])
    return st, tuple(o.value for o in out)


@pytest.mark.gpu
@pytest.mark.parametrize("case", INSTANCES, ids=[c["name"] for c in INSTANCES])
def test_every_instantiation_against_float64(case):
    from thunder_speech_amd import _lib
    st, (spt, threads, bp_lds, lds) = _query(_lib.lib(), case["n_frames"], case["s_max"])
    assert st == 0 and (spt, threads, bp_lds) == case["expect"], f"{case['name']}: the query says {(spt, threads, bp_lds)}, the row names {case['expect']}"
    if case["name"].endswith("big"):
        assert lds > 64 * 1024
    _run(case)


def test_every_instantiation_is_reached():
    """The six ctc_align_kernel instantiations are (states per thread) x (back-pointers in LDS or in the workspace); the rows above name each,
    and the host-only query agrees with every row (this part needs no GPU)."""
    from thunder_speech_amd import _lib
    assert {(c["expect"][0], c["expect"][2]) for c in INSTANCES} == {(s, l) for s in (1, 2, 4) for l in (0, 1)}
    for c in INSTANCES:
        st, got = _query(_lib.lib(), c["n_frames"], c["s_max"])
        assert st == 0 and (got[0], got[1], got[2]) == c["expect"], c["name"]


# ---- greedy spans --------------------------------------------------------------------------------------------------------------------------------
def _greedy_launch(logits, n, pitch, blank, lengths):
    from thunder_speech_amd import _lib
    L = _lib.lib()
    b, v = logits.shape[:2]
    lg = logits.cuda()
    il = None if lengths is None else torch.tensor(lengths, dtype=torch.int32).cuda()
    pad = 5
    tokens = torch.full((b * n + pad,), -77, dtype=torch.int32, device="cuda")
    spans = torch.full((b * n * 2 + pad,), -77, dtype=torch.int32, device="cuda")
    logp = torch.full((b * n + pad,), -77.0, device="cuda")
    counts = torch.full((b + pad,), -77, dtype=torch.int32, device="cuda")
    ws = torch.full((int(L.ts_ctc_greedy_spans_workspace_bytes(b, n)) + 16,), 0xFF, dtype=torch.uint8, device="cuda")
    st = L.ts_ctc_greedy_spans(lg.data_ptr(), b, v, n, pitch, None if il is None else il.data_ptr(), blank, tokens.data_ptr(), spans.data_ptr(),
                               logp.data_ptr(), counts.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert st == 0
    torch.cuda.synchronize()
    assert bool((ws[-16:] == 0xFF).all())
    for buf in (tokens, spans, logp, counts):
        assert bool((buf[-pad:] == -77).all())
    return (tokens[:-pad].view(b, n).cpu().numpy(), spans[:-pad].view(b, n, 2).cpu().numpy(), logp[:-pad].view(b, n).cpu().numpy(),
            counts[:-pad].cpu().numpy())


def _greedy_logits(seed, b, v, n, pitch, blank):
    """Random logits with planted structure: stretches where one class (often the blank) leads for several frames."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.full((b, v, pitch), float("nan"))
    logits[:, :, :n] = torch.randn(b, v, n, generator=g)
    for i in range(b):
        t = 0
        while t < n:
            run = int(torch.randint(1, 9, (1,), generator=g))
            cls = blank if float(torch.rand(1, generator=g)) < 0.4 else int(torch.randint(v, (1,), generator=g))
            logits[i, cls, t: min(t + run, n)] += 4.0
            t += run
    return logits


def _greedy_check(name, logits, n, blank, lengths, got):
    from thunder_speech_amd.module import greedy_decode
    tokens, spans, logp, counts = got
    for i in range(logits.shape[0]):
        T = n if lengths is None else max(0, min(lengths[i], n))
        ids = logits[i, :, :T].numpy().argmax(0) if T else np.zeros(0, np.int64)           # the lowest index wins ties
        lp = torch.log_softmax(logits[i, :, :T].double(), 0).numpy()
        runs = [r for r in _runs(ids) if r[0] != blank]
        c = int(counts[i])
        assert c == len(runs), f"{name}[{i}]: {c} spans, {len(runs)} runs"
        assert tokens[i, :c].tolist() == [r[0] for r in runs]
        assert spans[i, :c].tolist() == [[r[1], r[2]] for r in runs]
        assert (tokens[i, c:] == 0).all() and (spans[i, c:] == 0).all() and (logp[i, c:] == 0).all(), f"{name}[{i}]: entries beyond the count are not zero"
        if T:                                                          # ts_greedy_decode on the same frames: its collapsed ids with the blanks removed
            _, collapsed, cnt = greedy_decode(logits[i: i + 1, :, :T].contiguous().cuda())
            kept = [x for x in collapsed[0, : int(cnt[0])].cpu().tolist() if x != blank]
            assert kept == tokens[i, :c].tolist(), f"{name}[{i}]: tokens differ from ts_greedy_decode's"
        worst = 0.0
        for j, (tok, f0, f1) in enumerate(runs):
            want = float(lp[tok, f0:f1].sum())
            worst = max(worst, abs(float(logp[i, j]) - want) / (2 * T * U * abs(want)))
        print(f"RATIO|greedy-span-logp|{worst:.3e}|{name}[{i}] (T {T}, {c} spans)")
        assert worst <= 1.0, f"{name}[{i}]: span_logp off by {worst:.3e} of the bound"


@pytest.mark.gpu
@pytest.mark.parametrize("name,v,n,pitch,blank,lengths", [
    ("full", 29, 151, 160, 28, None),
    ("ragged", 29, 151, 160, 0, [151, 77, 1, 0, 900]),
    ("chunks", 8, 2500, 2500, 3, [2500, 1024, 1025, 2047, 1]),        # more than one chunk of 1 024 frames, and lengths on either side of a chunk
    ("one-frame", 5, 1, 4, 0, None),
])
def test_greedy_spans_against_numpy_and_ts_greedy_decode(name, v, n, pitch, blank, lengths):
    b = 5
    logits = _greedy_logits(21, b, v, n, pitch, blank)
    got = _greedy_launch(logits, n, pitch, blank, lengths)
    _greedy_check(name, logits, n, blank, lengths, got)


@pytest.mark.gpu
def test_greedy_spans_all_blank_and_a_clip_that_ends_inside_a_run():
    v, n, blank = 6, 40, 2
    logits = torch.randn(3, v, n, generator=torch.Generator().manual_seed(2))
    logits[0, blank] += 20.0                                           # all blank
    logits[1, 4, 10:30] += 20.0                                        # one long run; input_len 17 ends inside it
    logits[2, 1, :] += 20.0                                            # one run over the whole clip
    lengths = [40, 17, 40]
    got = _greedy_launch(logits, n, n, blank, lengths)
    _greedy_check("planted", logits, n, blank, lengths, got)
    tokens, spans, _, counts = got
    assert counts[0] == 0 and counts[2] == 1 and spans[2, 0].tolist() == [0, 40]
    assert tokens[1, counts[1] - 1] == 4 and spans[1, counts[1] - 1].tolist() == [10, 17]


@pytest.mark.gpu
def test_greedy_spans_agree_with_the_wav2vec2_tokenizer_char_offsets(tmp_path):
    transformers = pytest.importorskip("transformers")
    tokens = ["<pad>", "<s>", "</s>", "<unk>", "|"] + [chr(97 + i) for i in range(7)]
    vocab = tmp_path / "vocab.json"
    vocab.write_text(json.dumps({t: i for i, t in enumerate(tokens)}))
    try:
        tok = transformers.Wav2Vec2CTCTokenizer(str(vocab))
    except Exception as e:                                             # pragma: no cover
        pytest.skip(f"no offline Wav2Vec2CTCTokenizer: {e}")
    n = 120
    logits = _greedy_logits(8, 2, len(tokens), n, n, 0)
    tk, spans, _, counts = _greedy_launch(logits, n, n, 0, None)
    for i in range(2):
        out = tok.decode(logits[i].numpy().argmax(0).tolist(), output_char_offsets=True)
        want = [(" " if tokens[t] == "|" else tokens[t], int(f0), int(f1)) for t, (f0, f1) in zip(tk[i, : counts[i]], spans[i, : counts[i]])]
        assert [(o["char"], int(o["start_offset"]), int(o["end_offset"])) for o in out.char_offsets] == want


# ---- through the module --------------------------------------------------------------------------------------------------------------------------
def _quartznet():
    from oracle import tcs as otcs
    from thunder_speech_amd.quartznet.compatibility import build_synthetic_quartznet
    arch = otcs.quartznet_arch(repeat_blocks=1)
    module = build_synthetic_quartznet(repeat_blocks=1, encoder_state=otcs.synth_encoder_state(arch, seed=0, calibrate=True),
                                       decoder_state=otcs.synth_decoder_state(1024, 29, seed=1, gain=4.0))
    return module.cuda().eval(), 16000, 12000


def _wav2vec2(tmp_path):
    transformers = pytest.importorskip("transformers")
    from thunder_speech_amd.huggingface.compatibility import module_from_huggingface
    tokens = ["<pad>", "<s>", "</s>", "<unk>", "|"] + [chr(97 + i) for i in range(26)] + ["'"]
    vocab = tmp_path / "vocab.json"
    vocab.write_text(json.dumps({t: i for i, t in enumerate(tokens)}))
    tokenizer = transformers.Wav2Vec2CTCTokenizer(str(vocab))
    torch.manual_seed(3)
    cfg = transformers.Wav2Vec2Config(vocab_size=len(tokens), hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128,
                                      conv_dim=(32, 32, 32), conv_stride=(5, 2, 2), conv_kernel=(10, 3, 2), num_conv_pos_embeddings=16,
                                      num_conv_pos_embedding_groups=4, pad_token_id=0, mask_time_prob=0.0)
    model = transformers.Wav2Vec2ForCTC(cfg).eval()
    with torch.no_grad():
        model.lm_head.weight.mul_(20.0)                                # a head that prefers something: the greedy transcript is not empty
    module = module_from_huggingface(model, transformers.Wav2Vec2FeatureExtractor(return_attention_mask=True), tokenizer)
    return module.cuda().eval(), 8000, 6000


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["quartznet", "wav2vec2"])
def test_align_and_predict_spans_through_the_module(family, tmp_path):
    from thunder_speech_amd.ctc_align import forced_align, greedy_spans, words
    module, n0, n1 = _quartznet() if family == "quartznet" else _wav2vec2(tmp_path)
    spf, sr = module.samples_per_frame, module.sample_rate
    assert (spf, sr) == ((320, 16000) if family == "quartznet" else (20, 16000))
    rng = np.random.Generator(np.random.PCG64(7))
    wav = torch.from_numpy((0.1 * rng.standard_normal((2, n0))).astype(np.float32))
    wav[1, n1:] = 0
    x, lengths = wav.cuda(), torch.tensor([n0, n1]).cuda()
    texts = ["hello world", "abc"]
    blank = module.text_transform.vocab.blank_idx
    itos = module.text_transform.vocab.itos
    with torch.no_grad():
        logits, out_len = module(x, lengths)
    # align() = forced_align on the module's own logits and lengths
    clips = module.align(x, texts, lengths)
    y, y_len = module.text_transform.encode(texts, device=x.device)
    al = forced_align(logits, y, out_len, y_len, blank)
    spans, logp, score, ids, n_ids = [t.cpu().numpy() for t in (al.spans, al.span_logp, al.score, al.targets, al.target_lengths)]
    assert len(clips) == 2
    for b, clip in enumerate(clips):
        assert np.isfinite(score[b]) and abs(clip.score - float(score[b])) <= 1e-5 * abs(float(score[b]))
        assert len(clip.tokens) == int(n_ids[b]) == int(y_len[b])
        for j, tok in enumerate(clip.tokens):
            assert (tok.token, tok.start_frame, tok.end_frame) == (itos[ids[b, j]], int(spans[b, j, 0]), int(spans[b, j, 1]))
            assert abs(tok.logp - float(logp[b, j])) <= 1e-5 * abs(float(logp[b, j])) + 1e-7
            assert tok.start == tok.start_frame * spf / sr and tok.end == tok.end_frame * spf / sr
            assert 0 <= tok.start_frame < tok.end_frame <= int(out_len[b])
        assert [t.start_frame for t in clip.tokens] == sorted(t.start_frame for t in clip.tokens)
    assert [w.token for w in words(clips[0])] == ["hello", "world"]
    # a transcript that cannot fit: -inf and no tokens, the other clip is unharmed
    bad = module.align(x, ["a" * (int(out_len[0]) + 1), "abc"], lengths)
    assert bad[0].score == float("-inf") and bad[0].tokens == []
    assert [(t.token, t.start_frame, t.end_frame) for t in bad[1].tokens] == [(t.token, t.start_frame, t.end_frame) for t in clips[1].tokens]
    assert abs(bad[1].score - clips[1].score) <= 1e-5 * abs(clips[1].score)
    # predict_spans(): joining the tokens gives predict()
    greedy = module.predict_spans(x)
    with torch.no_grad():                                              # predict_spans() runs under no_grad itself; predict() follows the caller's mode
        want = module.predict(x)
    for b, clip in enumerate(greedy):
        text = "".join(t.token for t in clip.tokens).replace("▁", " ").replace("|", " ")
        assert module.text_transform.vocab.remove_special_tokens(text) == want[b]
        assert all(t.start == t.start_frame * spf / sr and t.end == t.end_frame * spf / sr for t in clip.tokens)
    assert family != "wav2vec2" or sum(len(c.tokens) for c in greedy) > 0
    # a clip aligned to its own greedy transcript: every aligned span contains the first frame of its greedy span
    full = torch.full((2,), logits.shape[2], dtype=torch.int32, device=x.device)
    gs = greedy_spans(logits, None, blank)
    counts = gs.counts.cpu()
    s = max(int(counts.max()), 1)
    self_al = forced_align(logits, gs.tokens[:, :s].contiguous(), full, gs.counts, blank)
    a_spans, g_spans = self_al.spans.cpu().numpy(), gs.spans.cpu().numpy()
    assert bool(torch.isfinite(self_al.score).all())
    for b in range(2):
        for j in range(int(counts[b])):
            assert a_spans[b, j, 0] <= g_spans[b, j, 0] < a_spans[b, j, 1], f"clip {b}, token {j}: aligned {a_spans[b, j]}, greedy {g_spans[b, j]}"
