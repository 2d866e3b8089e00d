"""ts_longform_gather, ts_longform_stitch and ts_ctc_align_long (csrc/longform.hip, csrc/ctc_align_long.hip; include_open/thunder_speech_amd/longform.h)
through the raw ABI.

Gather and stitch copy: they are compared bit for bit with numpy restatements, with sentinels around every output.

The aligner is checked by the method of tests/test_gpu_ctc_align.py against `_viterbi64` below: the Viterbi recursion over the blank-extended target on
log_softmax in float64, a Python loop over the frames with the states of a frame side by side in numpy, and the tie rule of the ABI (stay beats s-1,
s-1 beats s-2, the path ends in the last label state unless the final blank is strictly better).  Nothing of the package takes part in it.  Every case:
the kernel's path has length T, collapses to the target and is -1 beyond T; its score recomputed in float64 along that path and the `score` output
agree with the optimum within  2 T 2^-24  relative (that file's bound: the worst case of an f32 sum of T same-sign terms, each rounded once from f64,
with room for the normaliser); spans are the run boundaries of the kernel's own path and span_logp the float64 sums within the same bound.
Exact path equality is demanded where the test itself asserts that file's margin condition in float64 (the smallest gap between the best and the
second-best candidate along the optimal path exceeds  E = 3 T 2^-24 M,  M the largest magnitude of any partial path sum), where a single path is
feasible, and against ts_ctc_align on shapes both take (the same f32 recursion and tie rule).  The seeds of the margin cases were picked on the CPU;
the assertion of the condition stays in the test."""
import ctypes as C

import numpy as np
import pytest
import torch

U = 2.0 ** -24
NEG = -np.inf


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- gather --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("chunk,batch", [(1000, 8), (1003, 7)])           # 16-byte rows, and rows that are not
def test_gather_equals_numpy_slices_bit_for_bit(chunk, batch):
    from thunder_speech_amd import _lib
    L = _lib.lib()
    rng = np.random.Generator(np.random.PCG64(3))
    lengths = [chunk + 1, int(2.5 * chunk), 4 * chunk + 7]
    offset = 3                                                             # the packed buffer starts at an odd sample: no piece is 16-byte aligned by luck
    recs = [rng.standard_normal(n).astype(np.float32) for n in lengths]
    packed = np.concatenate([np.full(offset, np.nan, np.float32)] + recs + [np.full(5, np.nan, np.float32)])
    begin = np.cumsum([0] + lengths).astype(np.int64)
    # windows on either side of every end: inside, across the end (zero fill), wholly past it, and one with a wild recording index
    table = [(0, 0), (0, 1), (1, 4), (1, int(2.5 * chunk) - chunk + 8), (2, 3 * chunk + 7), (2, 4 * chunk + 40), (7, 0)][: batch - 1]
    n_win = len(table)
    pad = 16
    audio = torch.from_numpy(packed).cuda()
    out = torch.full((pad + batch * chunk + pad,), float("nan"), device="cuda")
    rb, wn = torch.from_numpy(begin).cuda(), torch.tensor(table + [(0, 0)], dtype=torch.int64).cuda()
    before = audio.clone()
    st = L.ts_longform_gather(audio.data_ptr() + 4 * offset, rb.data_ptr(), 3, wn.data_ptr(), n_win, out.data_ptr() + 4 * pad, batch, chunk, _stream())
    assert st == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    want = np.zeros((batch, chunk), np.float32)
    for i, (r, s) in enumerate(table):
        if 0 <= r < 3:
            piece = recs[r][s: s + chunk]
            want[i, : len(piece)] = piece
    assert np.isnan(got[:pad]).all() and np.isnan(got[-pad:]).all(), "cells around the output were written"
    assert np.array_equal(got[pad:-pad].view(np.int32), want.reshape(-1).view(np.int32))
    assert (want[n_win:] == 0).all() and np.abs(want[3]).sum() > 0 and (want[3, -7:] == 0).all() and (want[5] == 0).all()
    assert torch.equal(audio.view(torch.int32), before.view(torch.int32)), "the audio was written"


# ---- stitch --------------------------------------------------------------------------------------------------------------------------------------
def _coded(w, v, f, dtype):
    """Window "logits" that show where they came from.  f32: the value names (window, class, frame) exactly (below 2^24).  bf16 has 8 significant
    bits, too few for that: random values, so a cell taken from another window, class or frame differs almost surely."""
    if dtype == torch.bfloat16:
        return torch.randn(w, v, f, generator=torch.Generator().manual_seed(w * v)).to(dtype)
    wi, vi, fi = np.meshgrid(np.arange(w), np.arange(v), np.arange(f), indexing="ij")
    return torch.from_numpy((wi * 1e6 + vi * 1e3 + fi).astype(np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("v", [32, 1025])
def test_stitch_equals_its_numpy_restatement_bit_for_bit(v, dtype):
    from thunder_speech_amd import _lib
    from thunder_speech_amd.longform import cut_table, plan_windows
    L = _lib.lib()
    f, spf, chunk, ctx = 50, 320, 50 * 320 - 80, 6                        # hop 38 frames
    # 2 windows, the second nearly on top of the first; 1 "window" (a plan cannot have one: a hand-made row); 4 windows
    plans = [plan_windows(chunk + spf + 1, chunk, ctx, spf, f), None, plan_windows(3 * chunk + 11, chunk, ctx, spf, f)]
    assert [len(p) for p in plans if p] == [2, 4] and plans[0].frames == [0, 2]
    rows = cut_table(plans)
    rows = rows[:2] + [[1, 0, 0, 37]] + rows[2:]                           # recording 1: one window that owns frames [0, 37)
    n_win, n_rec = len(rows), 3
    t_max = max(r[3] for r in rows)
    pitch, pad = t_max + 9, 8
    win = _coded(n_win, v, f, dtype)
    out = torch.full((pad + n_rec * v * pitch + pad,), float("nan"), device="cuda")
    lengths = torch.full((n_rec + 2,), -77, dtype=torch.int32, device="cuda")
    cuts = torch.tensor(rows, dtype=torch.int32).cuda()
    wd = win.cuda()
    st = L.ts_longform_stitch(wd.data_ptr(), int(dtype == torch.bfloat16), n_win, v, f, cuts.data_ptr(), out.data_ptr() + 4 * pad, n_rec, pitch,
                              lengths.data_ptr(), _stream())
    assert st == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    src = win.float().numpy()
    want = np.zeros((n_rec, v, pitch), np.float32)
    owner = np.full((n_rec, pitch), -1)
    for w, (r, g, lo, hi) in enumerate(rows):
        want[r, :, lo:hi] = src[w, :, lo - g: hi - g]
        owner[r, lo:hi] = w
    assert np.isnan(got[:pad]).all() and np.isnan(got[-pad:]).all(), "cells around the output were written"
    assert np.array_equal(got[pad:-pad].view(np.int32), want.reshape(-1).view(np.int32))
    assert lengths.cpu().tolist() == [plans[0].n_frames, 37, plans[2].n_frames, -77, -77]
    # the fixture shows what it is meant to show: every frame below T_r has an owner, the second window of recording 0 owns from the seam on
    for r, t_r in enumerate([plans[0].n_frames, 37, plans[2].n_frames]):
        assert (owner[r, :t_r] >= 0).all() and (owner[r, t_r:] == -1).all() and (want[r, :, t_r:] == 0).all()
    assert plans[0].cut_hi[0] == (0 + f + 2) // 2 and owner[0, 25] == 0 and owner[0, 26] == 1


# ---- the float64 reference of the aligner ----------------------------------------------------------------------------------------------------------
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


def _target(g, s, v, blank, repeats):
    """s labels; repeats False: no two neighbours equal; a number: that many equal neighbours at random places, none elsewhere."""
    labels = np.array([i for i in range(v) if i != blank])
    out = labels[torch.randint(len(labels), (s,), generator=g).numpy()]
    for j in range(1, s):                                                  # no equal neighbours: move on to the next label
        if out[j] == out[j - 1]:
            out[j] = labels[(np.searchsorted(labels, out[j]) + 1) % len(labels)]
            if out[j] == out[j - 1]:
                out[j] = labels[(np.searchsorted(labels, out[j]) + 1) % len(labels)]
    if repeats and s > 1:
        for j in sorted(torch.randperm(s - 1, generator=g)[: int(repeats)].tolist()):
            out[j + 1] = out[j]
    return out.tolist()


def _case(name, v, blank, n_frames, s_max, utts, seed, spt=0, pitch=None, zero=False, equal=False):
    """utts: (input_len, target_len, repeats) per utterance, or (input_len, explicit target list)."""
    return dict(name=name, v=v, blank=blank, n_frames=n_frames, s_max=s_max, utts=utts, seed=seed, spt=spt, pitch=pitch or n_frames + 5, zero=zero,
                equal=equal)


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


def _launch(case, logits, targets, t_in, s_in, long=True):
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
    nbytes = int((L.ts_ctc_align_long_workspace_bytes if long else L.ts_ctc_align_workspace_bytes)(b, n, s_max))
    assert nbytes > 0
    ws = torch.full((nbytes + 16,), 0xFF, dtype=torch.uint8, device=dev)
    head = (lg.data_ptr(), b, v, n, case["pitch"], tg.data_ptr(), s_max, il.data_ptr(), tl.data_ptr(), case["blank"])
    tail = (path.data_ptr(), spans.data_ptr(), logp.data_ptr(), score.data_ptr(), ws.data_ptr(), _stream())
    st = L.ts_ctc_align_long(*head, case["spt"], *tail) if long else L.ts_ctc_align(*head, *tail)
    assert st == 0, f"{case['name']}: the aligner returned {st}"
    torch.cuda.synchronize()
    assert torch.equal(lg.view(torch.int32).cpu(), logits.view(torch.int32)), "the logits were written"
    assert bool((ws[-16:] == 0xFF).all()), "bytes beyond the workspace were written"
    for buf in (path, spans, logp, score):
        assert bool((buf[-pad:] == -77).all()), f"{case['name']}: cells behind an output were written"
    return (path[:-pad].view(b, n).cpu().numpy(), spans[:-pad].view(b, s_max, 2).cpu().numpy(), logp[:-pad].view(b, s_max).cpu().numpy(),
            score[:-pad].cpu().numpy())


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
        what = f"{case['name']}[{i}] (T {T}, S {S}, states_per_thread {case['spt']})"
        if ref["states"] is None:                                     # infeasible
            assert score[i] == NEG and (path[i] == -1).all() and (spans[i] == 0).all() and (logp[i] == 0).all(), what
            continue
        assert np.isfinite(score[i]), f"{what}: score {score[i]} for a feasible utterance"
        assert (path[i, T:] == -1).all() and (path[i, :T] >= 0).all() and (path[i, :T] < case["v"]).all(), what
        p = path[i, :T]
        heads = np.flatnonzero(np.concatenate([[True], p[1:] != p[:-1]])) if T else np.zeros(0, np.int64)
        ends = np.concatenate([heads[1:], [T]]).astype(np.int64) if T else heads
        keep = p[heads] != blank if T else np.zeros(0, bool)
        assert p[heads][keep].tolist() == target, f"{what}: the path does not collapse to the target"
        tol = 2 * max(T, 1) * U
        along = float(lp[p, np.arange(T)].sum())
        opt = ref["score"]
        print(f"RATIO|align-long-path|{(opt - along) / (tol * abs(opt)) if opt else 0.0:.3e}|{what} (optimum - score along the kernel's path) / (2 T u |optimum|)")
        print(f"RATIO|align-long-score|{abs(float(score[i]) - opt) / (tol * abs(opt)) if opt else abs(float(score[i])):.3e}|{what}")
        assert along >= opt - tol * abs(opt), f"{what}: the kernel's path scores {along}, the optimum is {opt}"
        assert abs(float(score[i]) - opt) <= tol * abs(opt), f"{what}: score {score[i]} against {opt}"
        assert (spans[i, S:] == 0).all() and (logp[i, S:] == 0).all(), what
        assert np.array_equal(spans[i, :S], np.stack([heads[keep], ends[keep]], 1)), f"{what}: the spans are not the runs of the kernel's own path"
        cum = np.concatenate([[0.0], np.cumsum(lp[p, np.arange(T)])])
        want = cum[ends[keep]] - cum[heads[keep]]
        exact = np.array([lp[target[j], f0:f1].sum() for j, (f0, f1) in enumerate(zip(heads[keep], ends[keep]))]) if S <= 300 else want
        worst = float(np.max(np.abs(logp[i, :S] - exact) / (tol * np.abs(exact)), initial=0.0))
        print(f"RATIO|align-long-span-logp|{worst:.3e}|{what}")
        assert worst <= 1.0, f"{what}: span_logp off by {worst:.3e} of the bound"
    return refs


def _run(case):
    built = _build(case)
    got = _launch(case, *built)
    return got, built, _check(case, got, *built)


def _path_of(states, target, blank):
    return _ext(target, blank)[states]


def _query(n_frames, s_max, spt_in, v):
    from thunder_speech_amd import _lib
    out = [C.c_int32(-7) for _ in range(3)]
    st = _lib.lib().ts_ctc_align_long_launch_config(n_frames, s_max, spt_in, v, *[C.addressof(o) for o in out])
    return st, tuple(o.value for o in out)


# ---- every instantiation, across the wave and workgroup boundaries --------------------------------------------------------------------------------
# 2 S + 1 states on either side of 64 threads' worth and into the third wave (a state count is odd: SPT 64 itself is not one); T = S + 40
def _boundary_cases():
    cases = []
    for spt in (8, 16, 32, 64):
        for states in (spt * 64 - 1, spt * 64 + 1, spt * 128 + 3):
            s = (states - 1) // 2
            cases.append(_case(f"spt{spt}-L{states}", 32, 0, s + 40, s, [(s + 40, s, 12)], seed=spt + states, spt=spt))
    return cases


BOUNDARY = _boundary_cases()


@pytest.mark.gpu
@pytest.mark.parametrize("case", BOUNDARY, ids=[c["name"] for c in BOUNDARY])
def test_every_instantiation_against_float64_across_the_wave_and_thread_boundaries(case):
    states = 2 * case["s_max"] + 1
    st, (spt, threads, lds) = _query(case["n_frames"], case["s_max"], case["spt"], case["v"])
    assert st == 0 and spt == case["spt"] and threads == (-(-states // spt) + 63) // 64 * 64
    assert threads == (64 if states < spt * 64 else (128 if states < spt * 128 else 192))
    _run(case)


# ---- edges ---------------------------------------------------------------------------------------------------------------------------------------
EDGES = [
    _case("s0-s1-t1", 5, 4, 16, 4, [(16, []), (1, [2]), (1, []), (0, []), (1, [1, 2]), (2, [3, 3]), (16, [1])], seed=4),
    _case("s-max-zero", 5, 0, 10, 0, [(10, []), (0, [])], seed=9),
    _case("infeasible", 6, 0, 20, 8, [(5, [1, 1, 2, 3]), (0, [2, 3]), (20, [1, 1, 2, 3]), (4, [1, 2, 3, 4, 5]), (-3, [1])], seed=3),
    # a ragged batch: input_len and target_len below the tensor's, one input_len beyond n_frames (clamped), blank in the middle, a wide pitch
    _case("ragged", 9, 3, 65, 16, [(65, 16, 3), (40, 7, 0), (17, 3, 0), (70, 5, 1)], seed=8, pitch=192),
    _case("ragged-spt64", 9, 8, 65, 40, [(65, 40, 2), (64, 16, 3), (17, 3, 0)], seed=8, spt=64),
    _case("v1025", 1025, 1024, 120, 50, [(120, 50, 5), (90, 20, 2)], seed=10),                 # the staging's overflow loop: V > 2 x 64 threads
    _case("v1025-spt16-wide", 1025, 0, 700, 600, [(700, 600, 20)], seed=11, spt=16),           # and V inside it: 128 threads x 2 registers < V ...
    _case("v1025-spt8-widest", 1025, 7, 2300, 2200, [(2300, 2200, 30)], seed=12, spt=8),       # ... and 576 threads x 2 >= V: registers alone
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", EDGES, ids=[c["name"] for c in EDGES])
def test_edges(case):
    _run(case)


@pytest.mark.gpu
@pytest.mark.parametrize("spt", [8, 64])
def test_one_repeated_label_has_a_single_feasible_path_and_none_one_frame_short(spt):
    """A target of one label r times needs r frames and r - 1 blanks between them: with T exactly that the path is fixed, whatever the logits."""
    r, v, blank, lab = 300, 6, 0, 4
    n = 2 * r - 1
    case = _case(f"single-path-spt{spt}", v, blank, n, r, [(n, [lab] * r), (n - 1, [lab] * r)], seed=20, spt=spt)
    got, built, refs = _run(case)
    want = np.full(n, blank)
    want[0::2] = lab
    assert np.array_equal(got[0][0], want) and np.array_equal(refs[0]["states"], np.arange(1, 2 * r, 1))
    assert refs[1]["states"] is None and got[3][1] == NEG and (got[0][1] == -1).all()


# ---- exact path equality under the margin condition ---------------------------------------------------------------------------------------------
# seeds picked on the CPU: of the seeds 0 .. 15 (0 .. 79 at T = 300) these have the widest margin / E at their shape
EQUAL = [
    _case("eq-t41", 5, 0, 41, 20, [(41, 20, 0)], seed=0, equal=True),
    _case("eq-t60", 8, 3, 60, 12, [(60, 12, 2)], seed=1, equal=True, spt=16),
    _case("eq-t200", 29, 28, 200, 40, [(200, 40, 3)], seed=7, equal=True, spt=32),
    _case("eq-t300", 6, 0, 300, 100, [(300, 100, 8)], seed=57, equal=True, spt=64),
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
    got, built, refs = _run(case)
    for i, (margin, e) in enumerate(_margin_condition(case, built, refs)):
        print(f"MARGIN|{case['name']}[{i}]|margin {margin:.3e}|E {e:.3e}")
        assert margin > e, f"{case['name']}: the fixture no longer meets the margin condition ({margin:.3e} <= {e:.3e}); pick another seed"
        T, S = int(built[2][i]), int(built[3][i])
        want = _path_of(refs[i]["states"], built[1][i, :S].tolist(), case["blank"])
        assert np.array_equal(got[0][i, :T], want), f"{case['name']}[{i}]: the path differs from the reference under the margin condition"


@pytest.mark.gpu
def test_tie_rule_fixes_the_path_on_all_zero_logits():
    """Every candidate is bit-equal in f32 and in f64, so the path is the rule's alone: stay, then s-1, then s-2; the last label state unless the
    final blank is strictly better."""
    case = _case("tie", 6, 2, 30, 7, [(30, [1, 3, 3, 4, 5, 1, 0]), (9, [1, 1, 3, 4]), (12, [])], seed=0, zero=True)
    got, built, refs = _run(case)
    for i, ref in enumerate(refs):
        T, S = int(built[2][i]), int(built[3][i])
        want = _path_of(ref["states"], built[1][i, :S].tolist(), case["blank"])
        assert np.array_equal(got[0][i, :T], want), f"tie[{i}]: {got[0][i, :T]} against {want}"


# ---- beyond the old cap, and against ts_ctc_align below it ----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_transcript_beyond_ts_ctc_aligns_cap():
    from thunder_speech_amd import _lib
    case = _case("auto-s2500", 32, 0, 6000, 2500, [(6000, 2500, 60)], seed=30)
    assert _lib.lib().ts_ctc_align_workspace_bytes(1, 6000, 2500) == _lib.TS_EUNSUPPORTED       # the refusal stays
    assert _query(6000, 2500, 0, 32) == (0, (8, 640, 64 * 32 + 8 * 641 + 80))
    _run(case)


@pytest.mark.gpu
@pytest.mark.parametrize("t,s,spt", [(200, 60, 0), (200, 60, 64), (999, 150, 0), (999, 150, 16)])
def test_path_and_spans_equal_ts_ctc_aligns_on_shapes_both_accept(t, s, spt):
    """The same f32 recursion on the raw logits and the same tie rule: the decisions are the same bits.  The sums differ by their order only."""
    case = _case(f"both-t{t}-s{s}", 32, 0, t, s, [(t, s, 4), (t - 30, s - 7, 0), (s // 2, s, 0)], seed=40 + t, spt=spt)
    built = _build(case)
    got = _launch(case, *built)
    old = _launch(case, *built, long=False)
    _check(case, got, *built)
    assert np.array_equal(got[0], old[0]) and np.array_equal(got[1], old[1])
    assert old[3][2] == NEG and got[3][2] == NEG                        # the third utterance is infeasible for both
    for i in range(2):
        T = int(built[2][i])
        tol = 2 * T * U
        tol = 2 * tol * (1 + tol)                                      # each is within the bound of the float64 value
        assert abs(float(got[3][i]) - float(old[3][i])) <= tol * abs(float(old[3][i]))
        assert np.all(np.abs(got[2][i] - old[2][i]) <= tol * np.abs(old[2][i]))
