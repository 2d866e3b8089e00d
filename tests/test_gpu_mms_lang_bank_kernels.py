"""The two launches of the MMS language bank on the GPU (csrc/mms_lang_bank.hip, include_open/thunder_speech_amd/mms_lang_bank.h):
ts_mms_lang_bank_adapter_fwd against ts_mms_attn_adapter_fwd run clip by clip with the slot's tensors (equal bits), ts_mms_lang_bank_head_fwd
against a float64 product, what neither may write, and every refusal of the header."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SENTINEL = 12345.0
N_SLOTS = 3


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t.data_ptr() if t is not None else None


# ---------------------------------------------------------------------------------------------------------------------
# 1. the adapter: equal bits with the single-language launch, clip by clip
# ---------------------------------------------------------------------------------------------------------------------
# t = 37 and t = 19 put clip boundaries inside what would be a flat 16-row tile; (1, 1, ..) is one partial tile; c = 1280 is the MMS-1B shape
ADAPTER_SHAPES = [(3, 37, 64, 16), (2, 16, 160, 32), (1, 1, 64, 16), (2, 19, 1280, 16)]
# three launches per case, so that every clip meets a mixed batch, a -1 and a stale 7 (both served by slot 0)
ID_PATTERNS = ([1, -1, 7], [7, 2, 1], [-1, 7, 2])

_ADAPTER_CASES = {}


def _adapter_case(batch, t, c, a, precision):
    """The banks, the input, and per (clip, slot) what ts_mms_attn_adapter_fwd writes for that clip's rows alone: computed once."""
    key = (batch, t, c, a, precision)
    if key in _ADAPTER_CASES:
        return _ADAPTER_CASES[key]
    from thunder_speech_amd import _lib
    L = _lib.lib()
    g = torch.Generator().manual_seed(batch + t + c + a + precision)
    dt = BF if precision else torch.float32
    rnd = lambda *s: torch.randn(*s, generator=g)
    k = dict(h=(2.0 * rnd(batch, t, c) + 0.5).cuda(), nw=(1.0 + 0.3 * rnd(N_SLOTS, c)).cuda(), nb=(0.2 * rnd(N_SLOTS, c)).cuda(),
             w1=(1.5 * rnd(N_SLOTS, a, c) / math.sqrt(c)).to(dt).cuda(), b1=(0.3 * rnd(N_SLOTS, a)).cuda(),
             w2=(0.5 * rnd(N_SLOTS, c, a)).to(dt).cuda(), b2=(0.3 * rnd(N_SLOTS, c)).cuda(),
             xw=(1.0 + 0.3 * rnd(c)).cuda(), xb=(0.2 * rnd(c)).cuda())
    ref = {}
    for b in range(batch):
        for s in range(N_SLOTS):
            h = k["h"][b].clone()
            y = torch.full((t, c), SENTINEL, device="cuda")
            y16 = torch.full((t, c), SENTINEL, dtype=BF, device="cuda") if precision else None
            st = L.ts_mms_attn_adapter_fwd(h.data_ptr(), t, c, a, k["nw"][s].data_ptr(), k["nb"][s].data_ptr(), k["w1"][s].data_ptr(),
                                           k["b1"][s].data_ptr(), k["w2"][s].data_ptr(), k["b2"][s].data_ptr(), k["xw"].data_ptr(),
                                           k["xb"].data_ptr(), 1e-3, y.data_ptr(), _ptr(y16), precision, _stream())
            assert st == 0
            ref[b, s] = (h, y, y16)
    torch.cuda.synchronize()
    # the slots differ: a launch that took another slot's tensors would not pass
    assert not torch.equal(ref[0, 0][0], ref[0, 1][0]) and not torch.equal(ref[0, 0][0], ref[0, 2][0])
    k["ref"] = ref
    _ADAPTER_CASES[key] = k
    return k


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("batch,t,c,a", ADAPTER_SHAPES)
def test_adapter_equals_the_single_language_launch_bit_for_bit(batch, t, c, a, precision):
    from thunder_speech_amd import _lib
    L = _lib.lib()
    k = _adapter_case(batch, t, c, a, precision)
    for pattern in ID_PATTERNS:
        ids = torch.tensor(pattern[:batch], dtype=torch.int32, device="cuda")
        # 16 rows behind the last in every buffer: a clip's partial last tile must not spill
        hbuf = torch.full((batch * t + 16, c), SENTINEL, device="cuda")
        hbuf[:batch * t] = k["h"].reshape(batch * t, c)
        y = torch.full((batch * t + 16, c), SENTINEL, device="cuda")
        y16 = torch.full((batch * t + 16, c), SENTINEL, dtype=BF, device="cuda") if precision else None
        st = L.ts_mms_lang_bank_adapter_fwd(hbuf.data_ptr(), batch, t, c, a, k["nw"].data_ptr(), k["nb"].data_ptr(), k["w1"].data_ptr(),
                                            k["b1"].data_ptr(), k["w2"].data_ptr(), k["b2"].data_ptr(), N_SLOTS, ids.data_ptr(), k["xw"].data_ptr(),
                                            k["xb"].data_ptr(), 1e-3, y.data_ptr(), _ptr(y16), precision, _stream())
        assert st == 0
        torch.cuda.synchronize()
        for buf in (hbuf, y, y16):
            if buf is not None:
                assert bool((buf[batch * t:] == SENTINEL).all()), "stored behind the last row"
        for b, i in enumerate(pattern[:batch]):
            s = i if 0 <= i < N_SLOTS else 0                             # -1 and the stale 7: slot 0
            want_h, want_y, want_y16 = k["ref"][b, s]
            rows = slice(b * t, (b + 1) * t)
            assert torch.equal(hbuf[rows], want_h), f"h of clip {b} (id {i})"
            assert torch.equal(y[rows], want_y), f"y_next of clip {b} (id {i})"
            if precision:
                assert torch.equal(y16[rows], want_y16), f"y_next_op of clip {b} (id {i})"


def test_adapter_without_the_layernorm_leaves_its_outputs_alone():
    from thunder_speech_amd import _lib
    batch, t, c, a = 3, 37, 64, 16
    k = _adapter_case(batch, t, c, a, 1)
    ids = torch.tensor([2, 0, 1], dtype=torch.int32, device="cuda")
    h = k["h"].clone()
    y = torch.full((batch * t, c), SENTINEL, device="cuda")
    st = _lib.lib().ts_mms_lang_bank_adapter_fwd(h.data_ptr(), batch, t, c, a, k["nw"].data_ptr(), k["nb"].data_ptr(), k["w1"].data_ptr(),
                                                 k["b1"].data_ptr(), k["w2"].data_ptr(), k["b2"].data_ptr(), N_SLOTS, ids.data_ptr(), None, None,
                                                 1e-3, y.data_ptr(), None, 1, _stream())
    assert st == 0
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all())
    for b, s in enumerate([2, 0, 1]):
        assert torch.equal(h[b], k["ref"][b, s][0])


def test_adapter_refuses_what_it_does_not_take():
    from thunder_speech_amd import _lib
    L = _lib.lib()
    c = 160
    h, v = torch.full((2, 4, c), SENTINEL, device="cuda"), torch.zeros(3 * c, device="cuda")
    w = torch.zeros(3 * 80 * c, device="cuda")
    y, y16 = torch.zeros(2, 4, c, device="cuda"), torch.zeros(2, 4, c, dtype=BF, device="cuda")
    ids = torch.zeros(4, dtype=torch.int32, device="cuda")

    def call(a=16, precision=0, next_w=None, next_b=None, yy=None, yy16=None, cc=c, hh=h, batch=2, t=4, n_slots=3, ii=ids, ii_off=0):
        return L.ts_mms_lang_bank_adapter_fwd(_ptr(hh), batch, t, cc, a, v.data_ptr(), v.data_ptr(), w.data_ptr(), v.data_ptr(), w.data_ptr(), v.data_ptr(),
                                              n_slots, (_ptr(ii) + ii_off) if ii is not None else None, _ptr(next_w), _ptr(next_b), 1e-5, _ptr(yy),
                                              _ptr(yy16), precision, _stream())
    E, U = _lib.TS_EINVAL, _lib.TS_EUNSUPPORTED
    # the existing launch's
    assert call(a=24) == U and call(a=80) == U and call(precision=2) == U and call(cc=156) == U
    assert call(next_w=v, next_b=v, yy=y, yy16=y16) == U               # y_next_op at precision 0
    assert call(next_w=v, next_b=v) == E and call(next_w=v, yy=y) == E
    assert call(hh=None) == E and call(a=0) == E and call(cc=0) == E
    assert L.ts_mms_lang_bank_adapter_fwd(h.data_ptr() + 4, 2, 4, c, 16, v.data_ptr(), v.data_ptr(), w.data_ptr(), v.data_ptr(), w.data_ptr(),
                                          v.data_ptr(), 3, ids.data_ptr(), None, None, 1e-5, None, None, 0, _stream()) == U
    # the bank's own
    assert call(n_slots=0) == E and call(ii=None) == E and call(batch=0) == E and call(t=0) == E and call(batch=-1) == E
    assert call(batch=65536) == U and call(ii_off=2) == U
    torch.cuda.synchronize()
    assert bool((h == SENTINEL).all()), "a refused call launched"
    assert L.ts_mms_lang_bank_abi_version() == 1


# ---------------------------------------------------------------------------------------------------------------------
# 2. the head against float64
# ---------------------------------------------------------------------------------------------------------------------
def _assert_bf16_product(got, ref, what):
    """tests/test_gpu_mms.py's bound for a bf16 product (copied): max <= 0.03 and rms <= 0.006 of max|ref|; a NaN fails."""
    got = got.detach().double().cpu()
    assert not bool(torch.isnan(got).any()), f"{what}: unwritten (NaN) elements"
    scale = float(ref.abs().max())
    mx, rms = float((got - ref).abs().max()), float((got - ref).pow(2).mean().sqrt())
    print(f"{what}: max {mx:.3e} rms {rms:.3e} against scale {scale:.3e}")
    assert mx <= 0.03 * scale and rms <= 0.006 * scale, f"{what}: max {mx:.3e} rms {rms:.3e} against scale {scale:.3e}"


def _assert_f32_product(got, ref, k, what):
    """tests/test_gpu_gemm_f32.py's bound for an f32 product of depth k (copied): 2e-6 sqrt(k) max|ref| + 1e-6."""
    got = got.detach().double().cpu()
    assert not bool(torch.isnan(got).any()), f"{what}: unwritten (NaN) elements"
    scale = float(ref.abs().max())
    err, tol = float((got - ref).abs().max()), 2e-6 * max(1, k ** 0.5) * scale + 1e-6
    print(f"{what}: max {err:.3e} against tolerance {tol:.3e} (scale {scale:.3e})")
    assert err <= tol, (what, err, tol)


def _run_head(h, w, bias, vocab, ids, v_pad, ldt, precision):
    from thunder_speech_amd import _lib
    b, t, c = h.shape
    buf = torch.full((b * v_pad * ldt + 64,), SENTINEL, device="cuda")
    st = _lib.lib().ts_mms_lang_bank_head_fwd(h.data_ptr(), b, t, c, w.data_ptr(), bias.data_ptr(), vocab.data_ptr(), vocab.numel(), v_pad,
                                              ids.data_ptr(), buf.data_ptr(), ldt, precision, _stream())
    assert st == 0
    torch.cuda.synchronize()
    return buf


# (batch, t, c, v_pad), the slots' vocabularies, the clips' ids: every slot is used; -1 and a stale 9 are slot 0
HEAD_CASES = [((3, 37, 64, 32), [7, 32, 20], [2, -1, 1]), ((2, 50, 1280, 160), [160, 33], [1, 9])]


@pytest.mark.parametrize("precision", [1, 0])
@pytest.mark.parametrize("shape,vocab,ids", HEAD_CASES)
def test_head_matches_float64(shape, vocab, ids, precision):
    batch, t, c, v_pad = shape
    n_slots = len(vocab)
    g = torch.Generator().manual_seed(sum(shape) + precision)
    dt = BF if precision else torch.float32
    h = torch.randn(batch, t, c, generator=g)
    w = (torch.randn(n_slots, v_pad, c, generator=g) / math.sqrt(c)).to(dt)
    bias = 0.5 * torch.randn(n_slots, v_pad, generator=g)
    ldt = (t + 3) // 4 * 4 + 4
    assert ldt > t
    d = dict(h=h.cuda(), w=w.cuda(), bias=bias.cuda(), vocab=torch.tensor(vocab, dtype=torch.int32, device="cuda"),
             ids=torch.tensor(ids, dtype=torch.int32, device="cuda"))
    buf = _run_head(d["h"], d["w"], d["bias"], d["vocab"], d["ids"], v_pad, ldt, precision)
    assert bool((buf[batch * v_pad * ldt:] == SENTINEL).all()), "stored behind the buffer"
    out = buf[:batch * v_pad * ldt].reshape(batch, v_pad, ldt)
    assert bool((out[:, :, t:] == SENTINEL).all()), "columns f >= t were written"
    hd = (h.to(BF) if precision else h).double()                         # precision 1 rounds h to bf16 in the kernel
    no_class = torch.tensor(-1e30, dtype=torch.float32)
    for b, i in enumerate(ids):
        s = i if 0 <= i < n_slots else 0
        n = vocab[s]
        want = bias[s, :n].double()[:, None] + w[s, :n].double() @ hd[b].T      # [n][t]
        got = out[b, :n, :t]
        what = f"head {shape} precision={precision} clip {b} slot {s}"
        if precision:
            _assert_bf16_product(got, want, what)
        else:
            _assert_f32_product(got, want, c, what)
        assert bool((out[b, n:, :t].cpu() == no_class).all()), f"{what}: classes >= {n} are not exactly -1e30f"
        # the clip alone, as a batch of one: equal bits
        alone = _run_head(d["h"][b:b + 1].contiguous(), d["w"], d["bias"], d["vocab"], d["ids"][b:b + 1].contiguous(), v_pad, ldt, precision)
        assert torch.equal(alone[:v_pad * ldt].reshape(v_pad, ldt), out[b]), f"{what}: differs from the clip run alone"


def test_head_counts_a_vocabulary_above_v_pad_as_v_pad():
    g = torch.Generator().manual_seed(5)
    h, w, bias = torch.randn(1, 5, 32, generator=g).cuda(), torch.randn(1, 16, 32, generator=g).to(BF).cuda(), torch.randn(1, 16, generator=g).cuda()
    ids = torch.zeros(1, dtype=torch.int32, device="cuda")
    big = _run_head(h, w, bias, torch.tensor([4000], dtype=torch.int32, device="cuda"), ids, 16, 8, 1)
    full = _run_head(h, w, bias, torch.tensor([16], dtype=torch.int32, device="cuda"), ids, 16, 8, 1)
    assert torch.equal(big, full) and bool((full[:16 * 8].reshape(16, 8)[:, :5] > -1e29).all())
    none = _run_head(h, w, bias, torch.tensor([0], dtype=torch.int32, device="cuda"), ids, 16, 8, 1)
    assert bool((none[:16 * 8].reshape(16, 8)[:, :5].cpu() == torch.tensor(-1e30, dtype=torch.float32)).all())


def test_head_refuses_what_it_does_not_take():
    from thunder_speech_amd import _lib
    L = _lib.lib()
    c, v_pad, t = 64, 32, 6
    h = torch.zeros(2, t, c, device="cuda")
    w, bias = torch.zeros(3, v_pad, c, dtype=BF, device="cuda"), torch.zeros(3, v_pad, device="cuda")
    vocab, ids = torch.full((3,), v_pad, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    out = torch.full((2 * v_pad * 8 + 8,), SENTINEL, device="cuda")
    args = dict(h=h, w=w, bias=bias, vocab=vocab, ids=ids, out=out)

    def call(batch=2, tt=t, cc=c, n_slots=3, vp=v_pad, ldt=8, precision=1, off=None, **none):
        p = {k: (None if none.get(k, "") is None else _ptr(a) + (off[1] if off and off[0] == k else 0)) for k, a in args.items()}
        return L.ts_mms_lang_bank_head_fwd(p["h"], batch, tt, cc, p["w"], p["bias"], p["vocab"], n_slots, vp, p["ids"], p["out"], ldt, precision,
                                           _stream())
    E, U = _lib.TS_EINVAL, _lib.TS_EUNSUPPORTED
    for name in args:
        assert call(**{name: None}) == E, name
    assert call(batch=0) == E and call(tt=0) == E and call(cc=0) == E and call(n_slots=0) == E and call(vp=0) == E and call(ldt=4) == E
    assert call(cc=48) == U and call(vp=24) == U and call(vp=4112) == U and call(batch=65536) == U and call(ldt=7) == U and call(precision=2) == U
    for name, by in (("h", 4), ("w", 2), ("bias", 4), ("out", 4), ("vocab", 2), ("ids", 2)):
        assert call(off=(name, by)) == U, name
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), "a refused call launched"
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out[2 * v_pad * 8:] == SENTINEL).all()) and bool((out[:2 * v_pad * 8].reshape(2, v_pad, 8)[:, :, :t] == 0).all())
