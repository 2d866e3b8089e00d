"""ts_ctc_loss (csrc/ctc.hip) through the C ABI, every instantiation of ctc_kernel asserted through ts_ctc_launch_config and compared with
torch.nn.functional.ctc_loss in float64 on the CPU.

Reference: log_softmax over the classes of logits[:, :, :max(input_len)] in float64, then F.ctc_loss -- reduction="none" for the per-utterance nll
(an infinite one is the 0 that zero_infinity stores), reduction="mean" with zero_infinity=True for the loss, and its autograd gradient with respect to
the logits for the gradient.  Lengths follow the header's rule: clamp(target_len, 0, s_max) labels are read, the mean divides by that count clamped
to at least 1.  Nothing of thunder_speech_amd or oracle takes part in the arithmetic.

Tolerance.  A worst-case bound on the log-domain recursion is useless (3 u32 T |alpha| is about 0.6 at T = 1300), so the yardstick is measured in every
case, on the same inputs: torch's own float32 CPU ctc_loss against the float64 one,
    e32[b] = max-norm error of its gradient for utterance b,          r32 = its largest relative nll error,
and the kernel must stay within  8 x e32[b]  per utterance and within  max(8 x r32, 4 u32)  relative on every nll and on the loss.  The margin of 8:
lse3_fast runs on the bare v_exp_f32 / v_log_f32 (1 ulp each, three exponentials and one log per state and step, against libm's correctly rounded
forms in torch), the association order of the three-way sum differs, and alpha and beta are stored as f32 rows and recombined with the emission and
the nll in a third kernel (one more exponential per state).  Every ratio is printed (`RATIO|kind|error / yardstick`; profiles/
frontend_ctc_se_kernel_checks.md records them); the assertions are ratio <= 8.

Exact checks: the gradient is exactly 0 for t >= input_len and for infeasible utterances; columns [n_frames, pitch) of the gradient buffer keep their
sentinel; the forward-only call (grad = NULL, one workgroup per utterance) returns the same nll and loss bits.  Logits beyond input_len are NaN, and
so is the whole workspace before the call: a read of either would show."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

NAN = float("nan")
U32 = 2.0 ** -24
SENTINEL = 7.0
MARGIN = 8.0


def _labels(g, n, classes, repeats):
    """n labels out of `classes`; repeats=False: no two neighbours alike (feasible from T = n on)"""
    if repeats:
        return [classes[int(i)] for i in torch.randint(0, len(classes), (n,), generator=g)]
    out, prev = [], None
    for i in torch.randint(0, len(classes) - 1, (n,), generator=g).tolist():
        pick = [c for c in classes if c != prev][i]
        out.append(pick)
        prev = pick
    return out


def _n_repeats(lab):
    return sum(1 for a, b in zip(lab, lab[1:]) if a == b)


def _case(name, v, blank, n_frames, s_max, utts, expect, pitch=None):
    """utts: (input_len, target_len, repeats) per utterance; expect: (states per thread, threads, lse row in LDS)"""
    return dict(name=name, v=v, blank=blank, n_frames=n_frames, pitch=pitch or n_frames, s_max=s_max, utts=utts, expect=expect)


CASES = [
    # ---- one state per thread: S = 0, T = 0 and S = 0, infeasible (25 frames for 20 labels with repeats), repeated labels
    _case("1-blank-mid-v8", 8, 3, 251, 40, [(251, 0, False), (0, 0, False), (25, 20, "infeasible"), (251, 40, True)], (1, 128, 1)),
    _case("1-blank-last-v9-pitch", 9, 8, 251, 40, [(251, 40, True), (200, 0, False), (0, 0, False), (25, 20, "infeasible")], (1, 128, 1), pitch=256),
    _case("1-v1", 1, 0, 251, 40, [(251, 0, False), (100, 0, False)], (1, 128, 1)),
    # ---- the thresholds of ctc_states_per_thread: 1023 states -> 1 per thread on 1024 threads, 1025 -> 2; 2047 -> 2, 2049 -> 4
    _case("threshold-511", 6, 0, 560, 511, [(560, 511, False), (543, 255, True)], (1, 1024, 1)),
    _case("threshold-512", 6, 5, 560, 512, [(560, 512, False), (543, 256, True)], (2, 576, 1)),
    _case("threshold-1023", 7, 2, 1080, 1023, [(1080, 1023, False), (1063, 511, True)], (2, 1024, 1)),
    _case("threshold-1024", 7, 6, 1080, 1024, [(1080, 1024, False), (1063, 512, True)], (4, 576, 1)),
    # ---- two and four states per thread
    _case("2-s600", 10, 4, 700, 600, [(700, 600, False), (699, 512, False), (300, 1, False)], (2, 640, 1)),
    _case("4-s1030", 12, 0, 1300, 1030, [(1300, 1030, False), (1299, 1024, False), (1000, 513, True), (700, 0, False)], (4, 576, 1)),
    _case("4-s2047", 6, 1, 2600, 2047, [(2600, 2047, False)], (4, 1024, 1)),
    # ---- more than 64 KiB of LDS: the tensor's time dimension selects the configuration, the work is input_len
    _case("biglds-2", 6, 2, 20000, 600, [(700, 600, False), (650, 300, True)], (2, 640, 1)),
    _case("biglds-4", 6, 5, 20000, 1030, [(700, 650, False)], (4, 576, 1)),
    # ---- the log-sum-exp row read back from global memory
    _case("lseglobal-1", 6, 0, 41000, 40, [(1300, 40, True)], (1, 128, 0)),
    _case("lseglobal-2", 6, 3, 41000, 600, [(1300, 600, False)], (2, 640, 0)),
    _case("lseglobal-4", 6, 5, 41000, 1030, [(1300, 1030, False)], (4, 576, 0)),
]


def _build(case, seed):
    g = torch.Generator().manual_seed(seed)
    v, blank, s_max, b = case["v"], case["blank"], case["s_max"], len(case["utts"])
    classes = [c for c in range(v) if c != blank]
    input_len = torch.tensor([u[0] for u in case["utts"]])
    target_len = torch.tensor([u[1] for u in case["utts"]])
    targets = torch.zeros(b, max(s_max, 1), dtype=torch.long)
    for i, (t, s, rep) in enumerate(case["utts"]):
        if s == 0:
            continue
        lab = _labels(g, s, classes, bool(rep))
        if rep == "infeasible":
            lab[1::2] = lab[0:-1:2]                                        # pairs of equal labels: s / 2 repeats
            assert t < s + _n_repeats(lab)
        else:
            assert t >= s + _n_repeats(lab), (case["name"], i, t, s, _n_repeats(lab))
        targets[i, :s] = torch.tensor(lab)
    t_max = max(int(input_len.max()), 1)
    logits = 2.0 * torch.randn(b, v, t_max, generator=g)
    return logits, targets, input_len, target_len


def _torch_ctc(logits, targets, input_len, target_len, blank, dtype):
    """(nll [B] with inf -> 0, mean loss, d loss / d logits [B][V][t_max]) on the CPU in `dtype`"""
    lg = logits.to(dtype).clone().requires_grad_(True)
    lp = F.log_softmax(lg, dim=1).permute(2, 0, 1)                         # [T][B][V]
    nll = F.ctc_loss(lp, targets, input_len, target_len, blank=blank, reduction="none")
    loss = F.ctc_loss(lp, targets, input_len, target_len, blank=blank, reduction="mean", zero_infinity=True)
    loss.backward()
    finite = torch.isfinite(nll.detach())
    nll = torch.where(finite, nll.detach(), torch.zeros_like(nll.detach()))
    return nll.double(), float(loss.detach().double()), lg.grad.double(), finite


def _query(L, n_frames, s_max):
    out = [C.c_int32(-7) for _ in range(4)]
    st = L.ts_ctc_launch_config(n_frames, s_max, *[C.byref(o) for o in out])
    return st, tuple(o.value for o in out)


def _launch(L, case, logits, targets, input_len, target_len, with_grad, s_max=None):
    b, v, n_frames, pitch = logits.shape[0], case["v"], case["n_frames"], case["pitch"]
    s_max = case["s_max"] if s_max is None else s_max
    dev = torch.full((b, v, pitch), NAN, device="cuda")
    for i, t in enumerate(input_len.tolist()):
        dev[i, :, :t] = logits[i, :, :t].cuda()
    tg = targets[:, :max(s_max, 1)].to(torch.int32).contiguous().cuda()
    il, tl = input_len.to(torch.int32).cuda(), target_len.to(torch.int32).cuda()
    ws_bytes = L.ts_ctc_workspace_bytes(b, v, n_frames, s_max)
    assert ws_bytes > 0
    ws = torch.full((ws_bytes,), 255, dtype=torch.uint8, device="cuda")    # every f32 of it a NaN
    nll = torch.full((b + 2,), SENTINEL, device="cuda")
    loss = torch.full((3,), SENTINEL, device="cuda")
    grad = torch.full((b, v, pitch), SENTINEL, device="cuda") if with_grad else None
    st = L.ts_ctc_loss(dev.data_ptr(), b, v, n_frames, pitch, tg.data_ptr(), s_max, il.data_ptr(), tl.data_ptr(), case["blank"], nll[1:].data_ptr(),
                       loss[1:].data_ptr(), grad.data_ptr() if with_grad else None, ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == 0, f"{case['name']}: ts_ctc_loss returned {st}"
    assert float(nll[0]) == SENTINEL and float(nll[b + 1]) == SENTINEL and float(loss[0]) == SENTINEL and float(loss[2]) == SENTINEL
    return nll[1: b + 1].cpu(), loss[1:2].cpu(), grad.cpu() if with_grad else None


def _compare(case, got, logits, targets, input_len, target_len):
    nll_k, loss_k, grad_k = got
    name, blank, n_frames = case["name"], case["blank"], case["n_frames"]
    b, v, t_max = logits.shape
    nll64, loss64, g64, feasible_or_empty = _torch_ctc(logits, targets, input_len, target_len, blank, torch.float64)
    nll32, loss32, g32, _ = _torch_ctc(logits, targets, input_len, target_len, blank, torch.float32)
    pos = nll64 > 0
    r32 = float(((nll32 - nll64).abs()[pos] / nll64[pos]).max()) if bool(pos.any()) else 0.0
    tol = max(MARGIN * r32, 4 * U32)
    e32 = (g32 - g64).abs().flatten(1).max(1).values
    err = (grad_k[:, :, :t_max].double() - g64).abs().flatten(1).max(1).values
    print(f"CALIB|{name}|r32={r32:.3e}|e32=" + ",".join(f"{float(x):.3e}" for x in e32) + f"|max|grad|={float(g64.abs().max()):.3e}")
    rel = (nll_k.double() - nll64).abs()[pos] / nll64[pos] if bool(pos.any()) else torch.zeros(1, dtype=torch.float64)
    rel_loss = abs(float(loss_k) - loss64) / loss64 if loss64 > 0 else abs(float(loss_k))
    ratios = [float(e / y) if y > 0 else (0.0 if e == 0 else float("inf")) for e, y in zip(err.tolist(), e32.tolist())]
    print(f"RATIO|ctc-nll|{float(rel.max()) / tol:.3e}|{name} (relative error / max(8 r32, 4 u32); in units of r32: "
          f"{float(rel.max()) / r32 if r32 > 0 else 0.0:.3e})")
    print(f"RATIO|ctc-loss|{rel_loss / tol:.3e}|{name}")
    print(f"RATIO|ctc-grad|{max(ratios):.3e}|{name} (error / e32 per utterance: " + ",".join(f"{r:.3e}" for r in ratios) + f"; the margin is {MARGIN:g})")
    assert not bool(torch.isnan(grad_k).any()) and not bool(torch.isnan(nll_k).any()) and not bool(torch.isnan(loss_k).any())
    assert bool((nll_k.double()[~pos] == 0).all()), f"{name}: nll of an empty or infeasible utterance is not 0"
    assert float(rel.max()) <= tol, f"{name}: nll off by {float(rel.max()):.3e} relative, allowed {tol:.3e}"
    assert rel_loss <= tol, f"{name}: loss {float(loss_k)} vs {loss64}, allowed {tol:.3e} relative"
    assert max(ratios) <= MARGIN, f"{name}: gradient error / e32 = {ratios}"
    # exact: zero from input_len to n_frames, zero for infeasible utterances, the sentinel from n_frames to the pitch
    for i, t in enumerate(input_len.tolist()):
        assert bool((grad_k[i, :, t:n_frames] == 0).all()), f"{name}: utterance {i}: gradient not exactly 0 from frame {t} on"
        if not bool(feasible_or_empty[i]):
            assert bool((grad_k[i, :, :n_frames] == 0).all()), f"{name}: infeasible utterance {i} has a gradient"
    assert bool((grad_k[:, :, n_frames:] == SENTINEL).all()), f"{name}: columns [n_frames, pitch) of the gradient were written"
    return r32, e32, ratios


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_ctc_loss_and_gradient_against_float64(case):
    from thunder_speech_amd import _lib
    L = _lib.lib()
    st, (spt, threads, lse_lds, lds) = _query(L, case["n_frames"], case["s_max"])
    lmax = 2 * case["s_max"] + 1
    assert st == 0 and (spt, threads, lse_lds) == case["expect"], f"{case['name']}: the query says {(spt, threads, lse_lds)}, the row names {case['expect']}"
    assert lds == 4 * (2 * (lmax + 4) + lmax + (case["n_frames"] if lse_lds else 0)) and threads * spt >= lmax
    if case["name"].startswith("biglds"):
        assert lds > 64 * 1024
    logits, targets, input_len, target_len = _build(case, seed=1 + CASES.index(case))
    got = _launch(L, case, logits, targets, input_len, target_len, True)
    _compare(case, got, logits, targets, input_len, target_len)
    # forward only: one workgroup per utterance, the same bits
    nll_f, loss_f, _ = _launch(L, case, logits, targets, input_len, target_len, False)
    assert torch.equal(nll_f.view(torch.int32), got[0].view(torch.int32)) and torch.equal(loss_f.view(torch.int32), got[1].view(torch.int32))


def test_every_instantiation_is_reached():
    """The six ctc_kernel instantiations are (states per thread) x (log-sum-exp row in LDS or global); the rows above name each of them, and the
    opt-in to more than 64 KiB of LDS is taken at 2 and at 4 states per thread."""
    assert {(c["expect"][0], c["expect"][2]) for c in CASES} == {(s, l) for s in (1, 2, 4) for l in (0, 1)}
    assert {c["expect"][0] for c in CASES if c["name"].startswith("biglds")} == {2, 4}


@pytest.mark.gpu
def test_s_max_zero_through_the_raw_abi():
    """s_max = 0: no label can be read, so target_len 0 and 3 both mean the empty transcript; the mean divides by clamp(target_len, 1, max(s_max, 1)) = 1
    for both, as the gradient does (ctc_mean_kernel used to divide by 0 here)."""
    from thunder_speech_amd import _lib
    L = _lib.lib()
    case = _case("s-max-0", 7, 2, 50, 0, [(50, 0, False), (37, 3, False)], (1, 64, 1))
    st, (spt, threads, lse_lds, lds) = _query(L, 50, 0)
    assert st == 0 and (spt, threads, lse_lds) == case["expect"]
    g = torch.Generator().manual_seed(77)
    logits = 2.0 * torch.randn(2, 7, 50, generator=g)
    targets = torch.zeros(2, 1, dtype=torch.long)
    input_len, target_len = torch.tensor([50, 37]), torch.tensor([0, 3])
    got = _launch(L, case, logits, targets, input_len, target_len, True)
    assert bool(torch.isfinite(got[1]).all()), f"loss = {float(got[1])}"
    _compare(case, got, logits, targets, input_len, target_len.clamp(max=0))


def test_launch_config_query_on_the_host():
    """ts_ctc_launch_config launches nothing and needs no device: thresholds, refusals, and the workspace it implies."""
    from thunder_speech_amd import _lib
    L = _lib.lib()
    E, U = _lib.TS_EINVAL, _lib.TS_EUNSUPPORTED
    for s_max in (0, 1, 40, 511, 512, 600, 1023, 1024, 1030, 2047):
        for n_frames in (1, 251, 20000, 38000, 41000):
            st, (spt, threads, lse_lds, lds) = _query(L, n_frames, s_max)
            lmax = 2 * s_max + 1
            want_spt = 1 if lmax <= 1024 else 2 if lmax <= 2048 else 4
            want_threads = ((lmax + want_spt - 1) // want_spt + 63) // 64 * 64
            with_row = 4 * (2 * (lmax + 4) + lmax + n_frames)
            assert st == 0 and (spt, threads) == (want_spt, want_threads) and threads <= 1024
            assert lse_lds == (1 if with_row <= 160 * 1024 else 0) and lds == (with_row if lse_lds else with_row - 4 * n_frames)
            rowp = spt * threads
            assert L.ts_ctc_workspace_bytes(3, 9, n_frames, s_max) == 2 * 4 * 3 * (n_frames + (n_frames + 1) * rowp) + 4 * 3
    assert _query(L, 251, 2048)[0] == U and _query(L, 0, 40)[0] == E and _query(L, -1, 40)[0] == E and _query(L, 251, -1)[0] == E
    assert _query(L, 251, 2048)[1] == (-7, -7, -7, -7)                     # a refusal writes nothing
    a = C.c_int32()
    assert L.ts_ctc_launch_config(251, 40, None, C.byref(a), C.byref(a), C.byref(a)) == E
    assert L.ts_ctc_launch_config(251, 40, C.byref(a), C.byref(a), C.byref(a), None) == E


@pytest.mark.gpu
def test_more_than_2047_labels_are_refused():
    from thunder_speech_amd import _lib
    L = _lib.lib()
    a = torch.zeros(4096, device="cuda").data_ptr()
    assert L.ts_ctc_loss(a, 1, 6, 100, 100, a, 2048, a, a, 0, a, a, a, a, None) == _lib.TS_EUNSUPPORTED
    assert L.ts_ctc_loss(a, 1, 6, 100, 100, a, 2047, a, a, 6, a, a, a, a, None) == _lib.TS_EINVAL           # blank outside the classes
    assert L.ts_ctc_loss(a, 1, 6, 100, 96, a, 40, a, a, 0, a, a, a, a, None) == _lib.TS_EINVAL              # pitch < n_frames
