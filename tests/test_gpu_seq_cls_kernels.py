"""The two entry points of the audio classification head on the GPU (csrc/seq_cls.hip, include_open/thunder_speech_amd/seq_cls.h) through the raw
C ABI, against a float64 restatement written here.

Bounds (derived, not measured): an f32 sum of n terms, in any order, is within n 2^-24 sum|terms| of the exact one; the restatement evaluates
that per element, with a factor 2 for the re-association, n = len + splits for the pool and n = c (projector) or p (classifier) for the head.
The classifier's bound also carries the projector's: |cls_w| times the bound of z."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SENTINEL = 12345.0
U = 2.0 ** -24


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _L():
    from thunder_speech_amd import _lib
    return _lib.lib()


def _config(t, c):
    s, r, blk = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    assert _L().ts_seq_cls_pool_launch_config(t, c, ctypes.byref(s), ctypes.byref(r), ctypes.byref(blk)) == 0
    return s.value, r.value, blk.value


def _pool(h, lens, w, accumulate, partials):
    b, t, c = h.shape
    st = _L().ts_seq_cls_pool(h.data_ptr(), b, t, c, _ptr(lens), _ptr(w), accumulate, partials.data_ptr(), _stream())
    assert st == 0
    torch.cuda.synchronize()


def _partials(batch, t, c):
    """The workspace with a sentinel tail behind it."""
    n = _L().ts_seq_cls_pool_workspace_bytes(batch, t, c) // 4
    assert n == batch * _config(t, c)[0] * c
    buf = torch.full((n + 64,), SENTINEL, device="cuda")
    return buf, n


# ---------------------------------------------------------------------------------------------------------------------
# 1. the pool
# ---------------------------------------------------------------------------------------------------------------------
def _lengths(batch, t):
    """1, t, 0 and something in between, as far as the batch goes (batch 1: the full clip); None stands for the NULL pointer."""
    return [t, 1, 0, max(1, t // 2), t - 1 if t > 1 else 1][:batch]


def _pool_ref(h64, lens, w):
    """(pooled f64 [b][c], sum of |terms| f64 [b][c]) of one call."""
    b, t, c = h64.shape
    pooled, mag = torch.zeros(b, c, dtype=torch.float64), torch.zeros(b, c, dtype=torch.float64)
    for i in range(b):
        n = t if lens is None else min(max(int(lens[i]), 0), t)
        if n:
            pooled[i] = w * h64[i, :n].sum(0) / n
            mag[i] = abs(w) * h64[i, :n].abs().sum(0) / n
    return pooled, mag


@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("c", [160, 1288])
@pytest.mark.parametrize("t", [1, 49, 130])
def test_pool_matches_float64_with_and_without_lengths_and_accumulates(t, c, batch):
    splits, rows, _ = _config(t, c)
    assert splits == {1: 1, 49: 2, 130: 5}[t]                          # below, off and across the split
    g = torch.Generator().manual_seed(1000 * t + c + batch)
    hs = [(torch.randn(batch, t, c, generator=g) + 0.3) for _ in range(3)]
    ws = [0.7, -1.3, 0.45]
    lens_host = _lengths(batch, t)
    lens = torch.tensor(lens_host, dtype=torch.int32, device="cuda")
    for use_len in (False, True):
        buf, n = _partials(batch, t, c)
        want, bound = torch.zeros(batch, c, dtype=torch.float64), torch.zeros(batch, c, dtype=torch.float64)
        for k, (h, w) in enumerate(zip(hs, ws)):
            wd = torch.tensor([w], device="cuda")
            _pool(h.cuda(), lens if use_len else None, wd, int(k > 0), buf)     # three device weights: the first call sets, the others accumulate
            w_eff = float(wd.item())
            p, mag = _pool_ref(h.double(), lens_host if use_len else None, w_eff)
            nn = torch.tensor([(min(l, t) if use_len else t) + splits for l in lens_host], dtype=torch.float64)[:, None]
            want += p
            bound += 2 * nn * U * mag
            got = buf[:n].view(batch, splits, c).double().sum(1).cpu()
            err = (got - want).abs()
            print(f"pool t={t} c={c} batch={batch} len={use_len} call {k}: max err {float(err.max()):.3e}, max err/bound "
                  f"{float((err / bound.clamp_min(1e-300)).max()):.3f}")
            assert bool((err <= bound).all())
        assert bool((buf[n:] == SENTINEL).all()), "stored behind the workspace"
        if use_len and batch >= 3:
            assert not bool(buf[:n].view(batch, splits, c)[2].any())    # len 0 pools to zeros, exactly
            # a split past the clip's length holds zeros: clip 1 has one frame
            assert splits == 1 or not bool(buf[:n].view(batch, splits, c)[1, 1:].any())


def test_pool_clamps_lengths_and_reads_the_weight_at_run_time():
    batch, t, c = 3, 49, 160
    g = torch.Generator().manual_seed(5)
    h = torch.randn(batch, t, c, generator=g).cuda()
    buf_a, n = _partials(batch, t, c)
    buf_b, _ = _partials(batch, t, c)
    _pool(h, torch.tensor([t + 7, -3, 1 << 30], dtype=torch.int32, device="cuda"), None, 0, buf_a)
    _pool(h, torch.tensor([t, 0, t], dtype=torch.int32, device="cuda"), None, 0, buf_b)
    assert torch.equal(buf_a, buf_b)
    w = torch.tensor([2.0], device="cuda")
    _pool(h, None, w, 0, buf_a)
    w.fill_(-0.5)                                                       # the same pointer, another value: what a replayed graph would see
    _pool(h, None, w, 0, buf_b)
    assert torch.equal(buf_a[:n] * -0.25, buf_b[:n])                   # scaling by powers of two is exact


# ---------------------------------------------------------------------------------------------------------------------
# 2. the head
# ---------------------------------------------------------------------------------------------------------------------
HEAD_SHAPES = [(160, 64, 12), (1280, 1024, 126), (1280, 1024, 4017)]
HEAD_T = 49                                                             # two splits: the head reduces them
MAX_BATCH = 33
_HEAD_CASES = {}


def _head_case(c, p, n_labels, precision):
    """Weights, partials of MAX_BATCH clips and the float64 restatement with its bounds: computed once per shape and precision, never changed."""
    key = (c, p, n_labels, precision)
    if key in _HEAD_CASES:
        return _HEAD_CASES[key]
    g = torch.Generator().manual_seed(c + p + n_labels + precision)
    rnd = lambda *s: torch.randn(*s, generator=g)
    splits = _config(HEAD_T, c)[0]
    dt = BF if precision else torch.float32
    k = dict(splits=splits, partials=(rnd(MAX_BATCH, splits, c) + 0.2), pw=(rnd(p, c) / math.sqrt(c)).to(dt), pb=0.1 * rnd(p),
             cw=(3.0 * rnd(n_labels, p) / math.sqrt(p)).to(dt), cb=0.1 * rnd(n_labels))
    # the restatement takes the weights as the kernel sees them: the bf16-rounded ones under precision 1
    x, pw, cw = k["partials"].double(), k["pw"].double(), k["cw"].double()
    pooled = x.sum(1)
    z = pooled @ pw.T + k["pb"].double()
    z_bound = 2 * c * U * (x.abs().sum(1) @ pw.abs().T + k["pb"].double().abs())
    logits = z @ cw.T + k["cb"].double()
    bound = 2 * p * U * (z.abs() @ cw.abs().T + k["cb"].double().abs()) + z_bound @ cw.abs().T
    k.update(z=z, logits=logits, bound=bound)
    k["dev"] = {n: k[n].cuda() for n in ("partials", "pw", "pb", "cw", "cb")}
    _HEAD_CASES[key] = k
    return k


def _head(k, batch, precision, class_slot=None, first=0, want_slot=True, cw=None, cb=None):
    """One ts_seq_cls_head call on clips [first, first + batch) -> (logits, top1, logp, slot) with sentinel tails checked."""
    L = _L()
    d = k["dev"]
    cw, cb = (d["cw"] if cw is None else cw), (d["cb"] if cb is None else cb)
    p, c = d["pw"].shape
    n = cw.shape[0]
    ws = torch.full((L.ts_seq_cls_head_workspace_bytes(batch, p) // 4 + 16,), SENTINEL, device="cuda")
    logits = torch.full((batch * n + 16,), SENTINEL, device="cuda")
    top1 = torch.full((batch + 4,), -77, dtype=torch.int32, device="cuda")
    logp = torch.full((batch + 4,), SENTINEL, device="cuda")
    slot = torch.full((batch + 4,), -77, dtype=torch.int32, device="cuda") if class_slot is not None else None
    part = d["partials"][first: first + batch].contiguous()
    st = L.ts_seq_cls_head(part.data_ptr(), batch, HEAD_T, c, d["pw"].data_ptr(), d["pb"].data_ptr(), p, cw.data_ptr(), cb.data_ptr(), n,
                           _ptr(class_slot), ws.data_ptr(), logits.data_ptr(), top1.data_ptr(), logp.data_ptr(), _ptr(slot), precision, _stream())
    assert st == 0
    torch.cuda.synchronize()
    assert bool((ws[batch * p:] == SENTINEL).all()) and bool((logits[batch * n:] == SENTINEL).all())
    assert bool((top1[batch:] == -77).all()) and bool((logp[batch:] == SENTINEL).all()) and (slot is None or bool((slot[batch:] == -77).all()))
    return logits[: batch * n].view(batch, n), top1[:batch], logp[:batch], (slot[:batch] if slot is not None else None)


def _first_argmax(x, allowed=None):
    """numpy's argmax: the first of equal maxima."""
    x = x.detach().cpu().numpy().astype(np.float64)
    if allowed is not None:
        x = np.where(allowed[None, :], x, -np.inf)
    return x.argmax(axis=1)


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("batch", [1, 16, 33])
@pytest.mark.parametrize("c,p,n_labels", HEAD_SHAPES)
def test_head_matches_float64(c, p, n_labels, batch, precision):
    k = _head_case(c, p, n_labels, precision)
    g = torch.Generator().manual_seed(n_labels)
    # about a third of the classes allowed, spread over 5 slots; the table is the same for every batch of a shape
    class_slot_host = torch.where(torch.rand(n_labels, generator=g) < 0.35, torch.randint(0, 5, (n_labels,), generator=g), torch.tensor(-1)).to(torch.int32)
    logits, top1, logp, slot = _head(k, batch, precision, class_slot_host.cuda())
    got = logits.double().cpu()
    want, bound = k["logits"][:batch], k["bound"][:batch]
    err = (got - want).abs()
    print(f"head c={c} p={p} L={n_labels} batch={batch} precision={precision}: max err {float(err.max()):.3e}, max err/bound "
          f"{float((err / bound).max()):.4f}, logit scale {float(want.abs().max()):.1f}")
    assert bool((err <= bound).all())
    # the arg-max is that of the launch's own logits, the first of equal maxima; and the restatement's wherever its margin exceeds the two classes' bounds
    assert top1.tolist() == _first_argmax(logits).tolist()
    top2 = want.topk(2, dim=1)
    clear = (top2.values[:, 0] - top2.values[:, 1]) > bound.gather(1, top2.indices).sum(1)
    assert torch.equal(top1.cpu().long()[clear], top2.indices[:, 0][clear])
    assert batch == 1 or bool(clear.any())                             # one clip's two best of 4017 random classes may lie within the bounds
    # log-softmax of the arg-max in f64 on the launch's logits.  exp(x - m) carries the rounding of x - m (relative |x - m| 2^-24 on a term
    # e^-(m - x): at most 0.37 2^-24 of the sum, which is >= 1) and a few ulp of expf; the n-term sum adds n 2^-24; logf a few ulp of its value
    ref_logp = torch.log_softmax(got, dim=1).gather(1, top1.cpu().long()[:, None])[:, 0]
    tol = 2 * (1.5 * n_labels + 8) * U + 4 * U * ref_logp.abs().clamp_min(1.0)
    assert bool(((logp.double().cpu() - ref_logp).abs() <= tol).all())
    allowed = (class_slot_host >= 0).numpy()
    v = _first_argmax(logits, allowed)
    assert slot.tolist() == class_slot_host[torch.from_numpy(v)].tolist()


def test_head_argmax_ties_go_to_the_lowest_index_and_the_restriction_is_honoured():
    c, p, n_labels = HEAD_SHAPES[0]
    batch = 16
    for precision in (0, 1):
        k = _head_case(c, p, n_labels, precision)
        base = _head(k, batch, precision)[0]
        win = _first_argmax(base)
        assert len(set(win.tolist())) > 1
        # duplicate every clip's winning row elsewhere: classes 3 and 9 become copies of the winners of clips 0 and 1 -- one copy below, one above
        cw, cb = k["dev"]["cw"].clone(), k["dev"]["cb"].clone()
        w0 = int(win[0])
        lo, hi = (w0 - 1 if w0 > 0 else None), (w0 + 1 if w0 + 1 < n_labels else None)
        for j in (lo, hi):
            if j is not None:
                cw[j], cb[j] = cw[w0], cb[w0]
        class_slot = torch.arange(n_labels, dtype=torch.int32, device="cuda")          # every class allowed: slot = the arg-max itself
        logits, top1, logp, slot = _head(k, batch, precision, class_slot, cw=cw, cb=cb)
        first = lo if lo is not None else w0
        if hi is not None:
            assert torch.equal(logits[:, hi], logits[:, w0])            # equal rows give equal bits
        assert int(top1[0]) == first and int(slot[0]) == first
        assert top1.tolist() == _first_argmax(logits).tolist() == slot.tolist()
        # the global winner disallowed: the best of the rest; every class disallowed: -1
        class_slot.copy_(torch.arange(100, 100 + n_labels, dtype=torch.int32))
        class_slot[int(top1[0])] = -1
        class_slot[int(top1[1])] = -1
        allowed = (class_slot >= 0).cpu().numpy()
        logits2, top1b, _, slot2 = _head(k, batch, precision, class_slot, cw=cw, cb=cb)
        assert torch.equal(logits2, logits) and torch.equal(top1b, top1)
        v = _first_argmax(logits, allowed)
        assert slot2.tolist() == (100 + v).tolist() and all(int(s) - 100 != int(t1) for s, t1 in zip(slot2, top1) if not allowed[int(t1)])
        assert any(not allowed[int(t1)] for t1 in top1)
        class_slot.fill_(-1)
        assert _head(k, batch, precision, class_slot, cw=cw, cb=cb)[3].tolist() == [-1] * batch
        class_slot.fill_(-5)
        class_slot[n_labels - 1] = 7                                    # one class allowed, far from any winner
        assert _head(k, batch, precision, class_slot, cw=cw, cb=cb)[3].tolist() == [7] * batch


@pytest.mark.parametrize("precision", [0, 1])
def test_equal_arguments_give_equal_bits_and_a_clip_depends_on_nothing_outside_it(precision):
    """Pool and head: the same call twice, and a 5-clip batch against each clip alone."""
    L = _L()
    batch, t, c, p, n_labels = 5, 130, 160, 64, 12
    k = _head_case(c, p, n_labels, precision)
    d = k["dev"]
    g = torch.Generator().manual_seed(77)
    h = torch.randn(batch, t, c, generator=g).cuda()
    lens = torch.tensor([130, 1, 0, 77, 129], dtype=torch.int32, device="cuda")
    w = torch.tensor([0.6], device="cuda")
    class_slot = torch.tensor([-1, 0, 1, -1, 2, 3, -1, -1, 4, 0, 1, -1], dtype=torch.int32, device="cuda")

    def chain(hh, ll):
        b = hh.shape[0]
        buf, n = _partials(b, t, c)
        _pool(hh, ll, None, 0, buf)
        _pool(hh.flip(1).contiguous(), ll, w, 1, buf)
        ws = torch.empty(L.ts_seq_cls_head_workspace_bytes(b, p), dtype=torch.uint8, device="cuda")
        logits, top1, logp, slot = torch.empty(b, n_labels, device="cuda"), torch.empty(b, dtype=torch.int32, device="cuda"), \
            torch.empty(b, device="cuda"), torch.empty(b, dtype=torch.int32, device="cuda")
        st = L.ts_seq_cls_head(buf.data_ptr(), b, t, c, d["pw"].data_ptr(), d["pb"].data_ptr(), p, d["cw"].data_ptr(), d["cb"].data_ptr(), n_labels,
                               class_slot.data_ptr(), ws.data_ptr(), logits.data_ptr(), top1.data_ptr(), logp.data_ptr(), slot.data_ptr(), precision,
                               _stream())
        assert st == 0
        torch.cuda.synchronize()
        return buf[:n].view(b, -1), logits, top1, logp, slot

    first, again = chain(h, lens), chain(h, lens)
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    assert bool(first[1].isfinite().all()) and not bool(first[0][2].any())
    for i in range(batch):
        alone = chain(h[i: i + 1].contiguous(), lens[i: i + 1].clone())
        for name, a, b in zip(("partials", "logits", "top1", "top1_logp", "slot"), first, alone):
            assert torch.equal(a[i: i + 1], b), f"{name} of clip {i}"


def test_every_refusal_of_the_header_with_real_buffers_and_nothing_written():
    from thunder_speech_amd import _lib
    L = _L()
    EI, EU = _lib.TS_EINVAL, _lib.TS_EUNSUPPORTED
    batch, t, c, p, n = 2, 49, 160, 64, 12
    h = torch.zeros(batch * t * c + 8, device="cuda")
    out = torch.full((batch * 2 * c + 8,), SENTINEL, device="cuda")
    lens, w = torch.zeros(batch + 1, dtype=torch.int32, device="cuda"), torch.ones(2, device="cuda")
    A = lambda x, off=0: x.data_ptr() + off
    pool = lambda hp=A(h), b=batch, tt=t, cc=c, ln=A(lens), wp=A(w), acc=0, op=A(out): L.ts_seq_cls_pool(hp, b, tt, cc, ln, wp, acc, op, _stream())
    assert [pool(hp=None), pool(op=None), pool(b=0), pool(tt=0), pool(cc=0), pool(acc=2)] == [EI] * 6
    assert [pool(cc=164), pool(cc=4104), pool(b=65536), pool(hp=A(h, 4)), pool(op=A(out, 8)), pool(ln=A(lens) + 2), pool(wp=A(w) + 1)] == [EU] * 7
    pw, pb, cw, cb = torch.zeros(p * c + 8, device="cuda"), torch.zeros(p + 1, device="cuda"), torch.zeros(n * p + 8, device="cuda"), torch.zeros(n + 1, device="cuda")
    ws, logits = torch.full((batch * p + 8,), SENTINEL, device="cuda"), torch.full((batch * n + 1,), SENTINEL, device="cuda")
    cs, top1, slot, logp = (torch.full((n + 1,), -1, dtype=torch.int32, device="cuda"), torch.full((batch + 1,), -77, dtype=torch.int32, device="cuda"),
                            torch.full((batch + 1,), -77, dtype=torch.int32, device="cuda"), torch.full((batch + 1,), SENTINEL, device="cuda"))
    good = dict(partials=A(out), batch=batch, t=t, c=c, pw=A(pw), pb=A(pb), p=p, cw=A(cw), cb=A(cb), n=n, cs=A(cs), ws=A(ws), logits=A(logits),
                top1=A(top1), logp=A(logp), slot=A(slot), prec=0)

    def head(**kw):
        a = {**good, **kw}
        return L.ts_seq_cls_head(a["partials"], a["batch"], a["t"], a["c"], a["pw"], a["pb"], a["p"], a["cw"], a["cb"], a["n"], a["cs"], a["ws"],
                                 a["logits"], a["top1"], a["logp"], a["slot"], a["prec"], _stream())
    assert [head(**{name: None}) for name in ("partials", "pw", "pb", "cw", "cb", "ws", "logits")] == [EI] * 7
    assert [head(**{name: 0}) for name in ("batch", "t", "c", "p", "n")] == [EI] * 5
    assert [head(cs=None), head(slot=None)] == [EI] * 2
    assert [head(c=164), head(c=4104), head(p=72), head(p=4112), head(n=8193), head(batch=65536), head(prec=2)] == [EU] * 7
    assert [head(**{name: good[name] + 8}) for name in ("partials", "pw", "cw", "ws")] == [EU] * 4
    assert [head(**{name: good[name] + 2}) for name in ("pb", "cb", "cs", "logits", "top1", "logp", "slot")] == [EU] * 7
    torch.cuda.synchronize()
    for buf, v in ((out, SENTINEL), (ws, SENTINEL), (logits, SENTINEL), (logp, SENTINEL), (top1, -77), (slot, -77)):
        assert bool((buf == v).all())                                   # no refused call launched anything
    assert head(top1=None, logp=None, cs=None, slot=None) == 0          # the optional outputs may all be absent
    torch.cuda.synchronize()
    assert bool((top1 == -77).all()) and bool((logits[: batch * n] != SENTINEL).all())
