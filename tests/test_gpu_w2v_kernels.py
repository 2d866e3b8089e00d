"""Every wav2vec2 encoder and fine-tuning kernel of csrc/w2v_conv.hip, w2v_rows.hip, w2v_posconv.hip, w2v_attn.hip, csrc/w2v_train.hip and csrc/w2v_attn_train.hip through the C ABI against a plain
float64 restatement on the CPU, at the shapes where the dispatch changes: the four register widths of the LayerNorms and a row that fills the last
register slot with one lane, the strided row loop of the LayerNorm backward, the generic conv-layer-0 instantiation, odd channel counts, the scalar
tails of the elementwise kernels, key lengths on and next to the 32- and 64-key tiles of both attention kernels.  Every output buffer starts as NaN (or
a sentinel next to a pitch) and every return code is asserted.  Inputs that are bf16 on the device are rounded first; the restatement reads the rounded
values.  The float64 restatements dominate the running time: the 380 cases take about 15 s next to an MI355X.

Bounds (one rule per kind of output):
  f32 elementwise / row-in-registers results (LayerNorm, softmax, column sums, conv layer 0)   1e-5 x max |reference|
  f32 products (conv layers, grouped conv, attention at precision 0)                          (2e-6 sqrt(contraction) + 1e-5) x max |reference| + 1e-6
  GELU forward / derivative                                                                   2e-6 absolute for |z| <= 8 (A&S 7.1.26: 1.5e-7 on erf, times |z| / 2 <= 4)
  bf16 copies of f32 results                                                                  bit-equal to the rounding of the f32 result
  bf16-operand products                                                                       max 0.03, rms 0.006 of max |reference|
  fused training attention                                                                    2e-2 relative L2 per output; per (32 rows x head) block and lse2: see below
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

NAN = float("nan")
BF = torch.bfloat16


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _api():
    from thunder_speech_amd import _lib
    return _lib, _lib.lib()


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def _ptr(x):
    return None if x is None else x.data_ptr()


def _ws(nbytes):
    assert nbytes >= 0
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device="cuda")


def _assert_close(got, ref, rel, what, extra=0.0):
    """max |got - ref| <= rel x max |ref| + extra; a NaN anywhere (an unwritten element) fails."""
    got = got.detach().double().cpu()
    assert not bool(torch.isnan(got).any()), f"{what}: unwritten (NaN) elements"
    err, scale = float((got - ref.double()).abs().max()), float(ref.abs().max())
    assert err <= rel * scale + extra, f"{what}: max error {err:.3e} > {rel:.1e} x {scale:.3e} + {extra:.1e}"


def _assert_bf16_product(got, ref, what):
    got = got.detach().double().cpu()
    assert not bool(torch.isnan(got).any()), f"{what}: unwritten (NaN) elements"
    scale = float(ref.abs().max())
    mx, rms = float((got - ref).abs().max()), float((got - ref).pow(2).mean().sqrt())
    assert mx <= 0.03 * scale and rms <= 0.006 * scale, f"{what}: max {mx:.3e} rms {rms:.3e} against scale {scale:.3e}"


def _gelu64(z):
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def _dgelu64(z):
    return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def _r4(n):
    return (n + 3) // 4 * 4


LN_C = [4, 64, 260, 512, 516, 768, 1024, 1028, 1280, 2048, 2052, 4096]      # NV = 2 | 4 | 8 | 16 at 512 | 1024 | 2048; 260, 516, 1028, 2052: one lane of the last slot


# ---------------------------------------------------------------------------------------------------------------------
# 1. LayerNorm
# ---------------------------------------------------------------------------------------------------------------------
def _ln_fwd_case(c, rows, offset, seed):
    _lib, L = _api()
    g = torch.Generator().manual_seed(seed)
    x = 2.0 * torch.randn(rows, c, generator=g) + offset                     # the mean is larger than the spread: the centred second pass matters
    res_h, xb_h = torch.randn(rows, c, generator=g), torch.randn(c, generator=g)
    w, b = 1.0 + 0.3 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g)
    dx, dres, dxb, dw, db = (z.cuda() for z in (x, res_h, xb_h, w, b))
    for use_res in (False, True):
        for use_xb in (False, True):
            s = x.double() + (res_h.double() if use_res else 0.0) + (xb_h.double() if use_xb else 0.0)
            ln = F.layer_norm(s, (c,), w.double(), b.double(), eps=1e-5)
            for act in (0, 1):
                ref = _gelu64(ln) if act else ln
                what = f"layernorm_fwd c={c} rows={rows} res={use_res} xbias={use_xb} act={act}"
                call = lambda y, y16: L.ts_w2v_layernorm_fwd(dx.data_ptr(), _ptr(dres) if use_res else None, _ptr(dxb) if use_xb else None, dw.data_ptr(),
                                                             db.data_ptr(), 1e-5, rows, c, act, _ptr(y), _ptr(y16), _stream())
                y_only, y_both, y16_both, y16_only = _nan(rows, c), _nan(rows, c), _nan(rows, c, dtype=BF), _nan(rows, c, dtype=BF)
                assert call(y_only, None) == 0 and call(y_both, y16_both) == 0 and call(None, y16_only) == 0
                torch.cuda.synchronize()
                _assert_close(y_only, ref, 1e-5, what)
                assert torch.equal(y_both, y_only), what
                # both stores come from the same registers
                assert torch.equal(y16_both.view(torch.int16), y_both.to(BF).view(torch.int16)), what + ": y_bf16 is not the rounding of y"
                assert torch.equal(y16_only.view(torch.int16), y16_both.view(torch.int16)), what + ": y_bf16 alone differs"


@pytest.mark.parametrize("rows", [1, 3, 6, 1001])                            # 1 and 3 leave idle waves in the last workgroup
@pytest.mark.parametrize("c", LN_C)
def test_layernorm_forward_matches_float64(c, rows):
    _ln_fwd_case(c, rows, 3.0, 7 * c + rows)


def test_layernorm_forward_with_a_mean_of_fifty_spreads():
    _ln_fwd_case(1028, 6, 100.0, 5)


def test_layernorm_forward_refuses_what_it_does_not_take():
    _lib, L = _api()
    buf = torch.zeros(4 * 4100 + 64, device="cuda")
    w = torch.ones(4100, device="cuda")
    y = torch.zeros(4 * 4100 + 64, device="cuda")
    call = lambda c, x=buf, yy=y, ww=w: L.ts_w2v_layernorm_fwd(x.data_ptr(), None, None, ww.data_ptr(), ww.data_ptr(), 1e-5, 4, c, 0, yy.data_ptr(), None, _stream())
    assert call(4096) == 0
    assert call(4100) == _lib.TS_EUNSUPPORTED and call(6) == _lib.TS_EUNSUPPORTED
    # float4 loads and stores: a pointer 4 bytes off a 16-byte boundary is refused on the host, before any launch (only the return code is looked at)
    assert call(64, x=buf[1:]) == _lib.TS_EUNSUPPORTED and call(64, yy=y[1:]) == _lib.TS_EUNSUPPORTED and call(64, ww=w[1:]) == _lib.TS_EUNSUPPORTED
    st = L.ts_w2v_layernorm_fwd(buf.data_ptr(), buf[1:].data_ptr(), None, w.data_ptr(), w.data_ptr(), 1e-5, 4, 64, 0, y.data_ptr(), None, _stream())
    assert st == _lib.TS_EUNSUPPORTED
    y16 = torch.zeros(1024, dtype=BF, device="cuda")
    st = L.ts_w2v_layernorm_fwd(buf.data_ptr(), None, None, w.data_ptr(), w.data_ptr(), 1e-5, 4, 64, 0, None, y16[1:].data_ptr(), _stream())
    assert st == _lib.TS_EUNSUPPORTED
    torch.cuda.synchronize()


# every c at 4097 rows (the strided row loop: wave 0 owns rows 0 and 4096); every row count at c = 260, 1024, 4096: 1, 2, 5 leave idle waves, 4095 is the
# last count with one row per wave, 9001 gives every wave two rows and some three
LN_BWD = sorted({(c, 4097) for c in LN_C} | {(c, r) for c in (260, 1024, 4096) for r in (1, 2, 5, 4095, 4096, 4097, 9001)})


@pytest.mark.parametrize("use_res", [False, True])
@pytest.mark.parametrize("c,rows", LN_BWD)
def test_layernorm_backward_matches_float64_autograd(c, rows, use_res):
    """dx, dgamma, dbeta of layer_norm(x + res) for ts_w2v_layernorm_bwd (dgamma / dbeta ADDED to random nonzero values) and ts_w2v_layernorm_bwd_set
    (written over NaN)."""
    _lib, L = _api()
    g = torch.Generator().manual_seed(3 * c + rows + use_res)
    x = 2.0 * torch.randn(rows, c, generator=g) + 3.0
    res = torch.randn(rows, c, generator=g) if use_res else None
    gamma, dy = 1.0 + 0.3 * torch.randn(c, generator=g), torch.randn(rows, c, generator=g)
    s = (x.double() + (res.double() if use_res else 0.0)).requires_grad_(True)
    gm, bt = gamma.double().requires_grad_(True), torch.zeros(c, dtype=torch.float64, requires_grad=True)
    F.layer_norm(s, (c,), gm, bt, eps=1e-5).backward(dy.double())
    r_dx, r_dg, r_db = s.grad, gm.grad, bt.grad
    del s
    dxx, dres, dgamma, ddy = x.cuda(), (res.cuda() if use_res else None), gamma.cuda(), dy.cuda()
    ws = _ws(L.ts_w2v_layernorm_bwd_workspace(rows, c))
    start_g, start_b = torch.randn(c, generator=g), torch.randn(c, generator=g)
    for fn, name, accumulate in ((L.ts_w2v_layernorm_bwd, "bwd", True), (L.ts_w2v_layernorm_bwd_set, "bwd_set", False)):
        dx = _nan(rows, c)
        dg, db = (start_g.cuda(), start_b.cuda()) if accumulate else (_nan(c), _nan(c))
        ws.fill_(0xFF)                                                       # NaN bit patterns: a partial row nobody wrote shows in the sums
        assert fn(dxx.data_ptr(), _ptr(dres), dgamma.data_ptr(), ddy.data_ptr(), 1e-5, rows, c, dx.data_ptr(), dg.data_ptr(), db.data_ptr(), ws.data_ptr(),
                  _stream()) == 0
        torch.cuda.synchronize()
        what = f"layernorm_{name} c={c} rows={rows} res={use_res}"
        _assert_close(dx, r_dx, 1e-5, what + " dx")
        base_g, base_b = (start_g.double(), start_b.double()) if accumulate else (0.0, 0.0)
        _assert_close(dg.double().cpu() - base_g, r_dg, 1e-5, what + " dgamma")
        _assert_close(db.double().cpu() - base_b, r_db, 1e-5, what + " dbeta")


# ---------------------------------------------------------------------------------------------------------------------
# 2. softmax, GELU and the small movers (csrc/w2v_train.hip)
# ---------------------------------------------------------------------------------------------------------------------
def _softmax_shapes():
    return [(t, p) for t in (1, 5, 63, 64, 65, 200) for p in sorted({t, _r4(t), t + 7})]


def _softmax_ref(s, n, scale):
    """s float64 [b][h][t][t], n [b] valid keys (already clamped to t): softmax over the first n keys, exactly 0 elsewhere, all zero for n <= 0."""
    t = s.shape[-1]
    pad = torch.arange(t)[None, :] >= n[:, None]
    z = (s * scale).masked_fill(pad[:, None, None, :], float("-inf"))
    p = torch.softmax(z, -1)
    return torch.where((n > 0)[:, None, None, None], p, torch.zeros_like(p))


@pytest.mark.parametrize("scale", [0.125, 1.0])
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("t,pitch", _softmax_shapes())
def test_training_softmax_forward_and_backward_match_float64(t, pitch, ragged, scale):
    """ts_w2v_softmax_fwd: keys >= key_len get exactly 0, a clip with key_len <= 0 is all zero (the header's convention), columns t .. pitch are zeroed.
    ts_w2v_softmax_bwd: scale p (dp - <dp, p>), columns t .. pitch zeroed."""
    _lib, L = _api()
    b, heads = 4, 2
    g = torch.Generator().manual_seed(100 * t + pitch + ragged)
    s = 4.0 * torch.randn(b, heads, t, t, generator=g)
    s[0, 1, t // 2, 0] += 80.0                                               # one row with an outlier: no overflow, the rest of the row underflows
    key_len = torch.tensor([t, 1, 0, t + 3], dtype=torch.int32) if ragged else None
    n = key_len.long().clamp(max=t) if ragged else torch.full((b,), t)
    ref = _softmax_ref(s.double(), n, scale)
    buf = _nan(b, heads, t, pitch)
    buf[..., :t] = s.cuda()
    kl = key_len.cuda() if ragged else None
    assert L.ts_w2v_softmax_fwd(buf.data_ptr(), _ptr(kl), b, heads, t, pitch, scale, _stream()) == 0
    torch.cuda.synchronize()
    what = f"softmax t={t} pitch={pitch} ragged={ragged} scale={scale}"
    _assert_close(buf[..., :t], ref, 1e-5, what + " fwd")
    got = buf.cpu()
    assert bool((got[..., t:] == 0).all()), what + ": columns t .. pitch"
    assert bool((got[..., :t][ref == 0] == 0).all()), what + ": a masked key has a nonzero probability"
    # backward on the reference's probabilities
    p32 = ref.float()
    dp = torch.randn(b, heads, t, t, generator=g)
    r_ds = scale * p32.double() * (dp.double() - (dp.double() * p32.double()).sum(-1, keepdim=True))
    pbuf, dbuf = _nan(b, heads, t, pitch), _nan(b, heads, t, pitch)
    pbuf[..., :t], dbuf[..., :t] = p32.cuda(), dp.cuda()
    assert L.ts_w2v_softmax_bwd(pbuf.data_ptr(), dbuf.data_ptr(), b * heads * t, t, pitch, scale, _stream()) == 0
    torch.cuda.synchronize()
    _assert_close(dbuf[..., :t], r_ds, 1e-5, what + " bwd", extra=1e-12)
    assert bool((dbuf[..., t:] == 0).all()), what + ": backward columns t .. pitch"


def _gelu_points(n, g):
    """n values spread over [-8, 8] in random order, the first ones 0, +-1e-4, +-8 as far as n allows."""
    z = torch.rand(n, generator=g) * 16.0 - 8.0
    special = torch.tensor([0.0, 8.0, -8.0, 1e-4, -1e-4])
    z[: min(n, 5)] = special[: min(n, 5)]
    return z


def _signed(shape, g):
    """+-(0.5 .. 2): an upstream gradient whose size is known elementwise"""
    return (0.5 + 1.5 * torch.rand(shape, generator=g)) * (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()


@pytest.mark.parametrize("n", [1, 3, 4, 1023, 1024 * 7 + 2])
def test_gelu_without_bias_and_its_scalar_tail_match_float64(n):
    _lib, L = _api()
    g = torch.Generator().manual_seed(n)
    z, dy = _gelu_points(n, g), _signed((n,), g)
    # a sentinel behind the n elements: the tail writes no more than n
    dz_, ddy = z.cuda(), dy.cuda()
    y, dz = _nan(n + 4), _nan(n + 4)
    assert L.ts_w2v_gelu_fwd(dz_.data_ptr(), None, 0, y.data_ptr(), n, _stream()) == 0
    assert L.ts_w2v_gelu_bwd(dz_.data_ptr(), None, 0, ddy.data_ptr(), dz.data_ptr(), n, _stream()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(y[n:]).all()) and bool(torch.isnan(dz[n:]).all())
    assert not bool(torch.isnan(y[:n]).any()) and not bool(torch.isnan(dz[:n]).any())
    assert float((y[:n].double().cpu() - _gelu64(z.double())).abs().max()) <= 2e-6
    err = (dz[:n].double().cpu() - dy.double() * _dgelu64(z.double())).abs()
    assert bool((err <= 2e-6 * dy.double().abs()).all()), float((err / dy.double().abs()).max())


@pytest.mark.parametrize("c", [4, 260, 4096])
def test_gelu_with_a_column_bias_matches_float64(c):
    _lib, L = _api()
    rows = 7
    g = torch.Generator().manual_seed(c)
    bias = torch.randint(-4, 5, (c,), generator=g).float() / 4.0             # multiples of 1 / 4 in [-1, 1]
    bias[0] = 0.0                                                            # column 0 carries 0, +-8, +-1e-4 exactly
    tot = torch.rand(rows, c, generator=g) * 15.8 - 7.9
    tot[:5, 0] = torch.tensor([0.0, 8.0, -8.0, 1e-4, -1e-4])
    z = tot - bias
    arg = (z + bias).double()                                                # the f32 sum the kernel forms (one IEEE add), then float64
    assert float(arg.abs().max()) <= 8.0 and set(arg[:5, 0].tolist()) == {0.0, 8.0, -8.0, float(torch.tensor(1e-4)), float(torch.tensor(-1e-4))}
    dy = _signed((rows, c), g)
    dz_, db, ddy = z.cuda(), bias.cuda(), dy.cuda()
    y, dz = _nan(rows, c), _nan(rows, c)
    assert L.ts_w2v_gelu_fwd(dz_.data_ptr(), db.data_ptr(), c, y.data_ptr(), rows * c, _stream()) == 0
    assert L.ts_w2v_gelu_bwd(dz_.data_ptr(), db.data_ptr(), c, ddy.data_ptr(), dz.data_ptr(), rows * c, _stream()) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(y).any()) and not bool(torch.isnan(dz).any())
    assert float((y.double().cpu() - _gelu64(arg)).abs().max()) <= 2e-6
    err = (dz.double().cpu() - dy.double() * _dgelu64(arg)).abs()
    assert bool((err <= 2e-6 * dy.double().abs()).all()), float((err / dy.double().abs()).max())


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("c", [4, 68, 1024])
@pytest.mark.parametrize("rows", [1, 63, 65, 130])
def test_ffn_activation_cast_and_its_backward_match_float64_and_the_oracle_mask(rows, c, p):
    """ts_w2v_ffn_act_cast: bf16(dropout(gelu(z + bias))) and its transposed, zero-padded copy; ts_w2v_ffn_act_bwd: dropout'(da) gelu'(z + bias).  The keep
    mask is the oracle's Philox stream.  Bounds: the bf16 result is within half a bf16 ulp (2^-8 relative) of the reference plus the f32 value's own
    error, 2e-6 / (1 - p) for the GELU and one rounding of the scaling (below 3e-6 in all for |gelu| <= 8); the f32 gradient within 2e-6 |da| / (1 - p) for
    the derivative plus two f32 roundings (2.2e-6 |da| / (1 - p) in all)."""
    from oracle import philox as ph
    _lib, L = _api()
    seed = 424242 + rows
    g = torch.Generator().manual_seed(rows * c + int(10 * p))
    bias = torch.randint(-4, 5, (c,), generator=g).float() / 4.0
    z = (2.0 * torch.randn(rows, c, generator=g)).clamp(-7.0, 7.0)
    arg = (z + bias).double()
    keep = torch.from_numpy(ph.dropout_keep(seed, rows * c, p)).view(rows, c) if p > 0 else torch.ones(rows, c, dtype=torch.bool)
    ref = _gelu64(arg) * keep.double() / (1.0 - p)
    rp = (rows + 31) // 32 * 32
    ldt = rp + 2
    dz_, db = z.cuda(), bias.cuda()
    sentinel = 7.0

    def run(want_y, want_t):
        y = _nan(rows, c, dtype=BF) if want_y else None
        yt = torch.full((c, ldt), sentinel, dtype=BF, device="cuda") if want_t else None
        assert L.ts_w2v_ffn_act_cast(dz_.data_ptr(), db.data_ptr(), rows, c, p, seed, _ptr(y), _ptr(yt), ldt if want_t else 0, rp if want_t else rows,
                                     _stream()) == 0
        torch.cuda.synchronize()
        return y, yt

    def check(got, what):
        got = got.double().cpu()
        assert not bool(torch.isnan(got).any()), what
        assert bool((got[~keep] == 0).all()), what + ": a dropped element is not zero"
        err = (got - ref).abs()
        assert bool((err <= 2.0 ** -8 * ref.abs() + 3e-6).all()), (what, float((err - 2.0 ** -8 * ref.abs()).max()))

    outs = []
    for want_y, want_t in ((True, False), (False, True), (True, True)):
        y, yt = run(want_y, want_t)
        what = f"ffn_act_cast rows={rows} c={c} p={p} y={want_y} yt={want_t}"
        if want_y:
            check(y, what + " y")
            outs.append(y)
        if want_t:
            check(yt[:, :rows].t(), what + " yt")
            assert bool((yt[:, rows:rp].float() == 0).all()), what + ": rows .. rows_pad of the transposed copy"
            assert bool((yt[:, rp:].float() == sentinel).all()), what + ": written beyond rows_pad"
            outs.append(yt[:, :rows].t().contiguous())
    for o in outs[1:]:                                                       # one arithmetic, four stores
        assert torch.equal(o.view(torch.int16), outs[0].view(torch.int16))
    da = _signed((rows, c), g)
    dda, dz = da.cuda(), _nan(rows, c)
    assert L.ts_w2v_ffn_act_bwd(dz_.data_ptr(), db.data_ptr(), c, dda.data_ptr(), p, seed, dz.data_ptr(), rows * c, _stream()) == 0
    torch.cuda.synchronize()
    r_dz = da.double() * keep.double() / (1.0 - p) * _dgelu64(arg)
    got = dz.double().cpu()
    assert not bool(torch.isnan(got).any())
    assert bool((got[~keep] == 0).all())
    assert bool(((got - r_dz).abs() <= 2.2e-6 * da.double().abs() / (1.0 - p)).all()), float(((got - r_dz).abs() / da.double().abs()).max())


@pytest.mark.parametrize("rows,c,ldx", [(70, 31, 32), (65, 68, 68)])         # the element path (odd c, odd pitch); the vector path with a partial tile both ways
def test_cast_with_column_sums_on_both_paths(rows, c, ldx):
    _lib, L = _api()
    g = torch.Generator().manual_seed(rows + c)
    x = torch.randn(rows, ldx, generator=g)
    start = torch.randn(c, generator=g)
    rp = (rows + 31) // 32 * 32
    ldt = rp + 2
    dx, cs = x.cuda(), start.cuda()
    y = _nan(rows, c, dtype=BF)
    yt = torch.full((c, ldt), 7.0, dtype=BF, device="cuda")
    assert L.ts_w2v_cast_bf16_t_colsum(dx.data_ptr(), ldx, rows, c, y.data_ptr(), c, yt.data_ptr(), ldt, rp, cs.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    want = x[:, :c].to(BF)
    assert torch.equal(y.cpu().view(torch.int16), want.view(torch.int16))
    assert torch.equal(yt[:, :rows].cpu().view(torch.int16), want.t().contiguous().view(torch.int16))
    assert bool((yt[:, rows:rp].float() == 0).all()) and bool((yt[:, rp:].float() == 7.0).all())
    _assert_close(cs, start.double() + x[:, :c].double().sum(0), 1e-5, f"cast colsum rows={rows} c={c}")


@pytest.mark.parametrize("c", [1, 63, 64, 65, 1024])
@pytest.mark.parametrize("rows", [1, 15, 16, 17, 4095, 4096, 5000])
def test_column_sums_are_added_to_a_nonzero_output(rows, c):
    _lib, L = _api()
    for ld in (c, c + 3):
        g = torch.Generator().manual_seed(rows + c + ld)
        x, start = torch.randn(rows, ld, generator=g), torch.randn(c + 2, generator=g)
        dx, out = x.cuda(), start.cuda()
        assert L.ts_w2v_colsum(dx.data_ptr(), rows, c, ld, out.data_ptr(), _stream()) == 0
        torch.cuda.synchronize()
        _assert_close(out[:c], start[:c].double() + x[:, :c].double().sum(0), 1e-5, f"colsum rows={rows} c={c} ld={ld}")
        assert torch.equal(out[c:].cpu(), start[c:])                         # nothing added beyond c


@pytest.mark.parametrize("n_parts", [1, 2, 8])
def test_split_k_parts_are_summed_in_part_order(n_parts):
    _lib, L = _api()
    rows, c = 37, 68
    n = rows * c
    g = torch.Generator().manual_seed(n_parts)
    parts, bias = torch.randn(n_parts, rows, c, generator=g) * 100.0, torch.randn(c, generator=g)
    acc = parts[0].clone()
    for i in range(1, n_parts):
        acc = acc + parts[i]                                                 # float32, the kernel's fixed order
    dparts, dbias = parts.cuda(), bias.cuda()
    out, outb = _nan(rows, c), _nan(rows, c)
    assert L.ts_w2v_sum_parts(dparts.data_ptr(), out.data_ptr(), n, n_parts, _stream()) == 0
    assert L.ts_w2v_sum_parts_bias(dparts.data_ptr(), dbias.data_ptr(), c, outb.data_ptr(), n, n_parts, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), acc)
    assert torch.equal(outb.cpu(), acc + bias)
    _assert_close(out, parts.double().sum(0), 1e-5, "sum_parts")
    _assert_close(outb, parts.double().sum(0) + bias.double(), 1e-5, "sum_parts_bias")


@pytest.mark.parametrize("left", [0, 3])
@pytest.mark.parametrize("extra", [0, 5])
def test_pad_rows_moves_clips_both_ways(left, extra):
    _lib, L = _api()
    b, t, c = 3, 7, 12
    t_dst = t + left + extra
    g = torch.Generator().manual_seed(left + extra)
    src = torch.randn(b, t, c, generator=g)
    dst = _nan(b, t_dst, c)
    assert L.ts_w2v_pad_rows(src.cuda().data_ptr(), dst.data_ptr(), b, t, t_dst, left, c, 0, _stream()) == 0
    want = torch.zeros(b, t_dst, c)
    want[:, left:left + t] = src
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), want)
    big = torch.randn(b, t_dst, c, generator=g)
    out = _nan(b, t, c)
    assert L.ts_w2v_pad_rows(big.cuda().data_ptr(), out.data_ptr(), b, t, t_dst, left, c, 1, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), big[:, left:left + t])


def test_mask_rows_zeroes_the_rows_behind_each_length():
    _lib, L = _api()
    t, c = 6, 10
    lens = [0, 1, t, t + 3, -2]
    x = torch.randn(len(lens), t, c, generator=torch.Generator().manual_seed(1)) + 5.0
    dx, dl = x.cuda(), torch.tensor(lens, dtype=torch.int32).cuda()
    assert L.ts_w2v_mask_rows(dx.data_ptr(), len(lens), t, c, dl.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    want = x.clone()
    for i, n in enumerate(lens):
        want[i, max(0, min(n, t)):] = 0
    assert torch.equal(dx.cpu(), want)


@pytest.mark.parametrize("which", ["none", "all", "third"])
def test_mask_embed_forward_and_backward(which):
    _lib, L = _api()
    b, t, c = 3, 50, 260
    rows = b * t
    g = torch.Generator().manual_seed(len(which))
    mask = {"none": torch.zeros(rows), "all": torch.ones(rows), "third": (torch.rand(rows, generator=g) < 1 / 3).float()}[which].to(torch.uint8)
    x, embed, start = torch.randn(rows, c, generator=g), torch.randn(c, generator=g), torch.randn(c, generator=g)
    dx, dm, de = x.cuda(), mask.cuda(), embed.cuda()
    assert L.ts_w2v_mask_embed(dx.data_ptr(), dm.data_ptr(), de.data_ptr(), None, rows, c, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(dx.cpu(), torch.where(mask.bool()[:, None], embed[None, :], x))
    dy, dembed = x.cuda(), start.cuda()
    assert L.ts_w2v_mask_embed(dy.data_ptr(), dm.data_ptr(), None, dembed.data_ptr(), rows, c, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(dy.cpu(), torch.where(mask.bool()[:, None], torch.zeros_like(x), x))
    want = start.double() + x.double()[mask.bool()].sum(0)
    _assert_close(dembed, want, 1e-5, f"mask_embed dembed ({which})")
    if which == "none":
        assert torch.equal(dembed.cpu(), start)


@pytest.mark.parametrize("n", [1, 5, 4096 + 3])
def test_add_and_its_scalar_tail(n):
    _lib, L = _api()
    g = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    y = _nan(n + 4)
    assert L.ts_w2v_add(a.cuda().data_ptr(), b.cuda().data_ptr(), y.data_ptr(), n, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(y[:n].cpu(), a + b) and bool(torch.isnan(y[n:]).all())


@pytest.mark.parametrize("c", [4, 260])
def test_glu_matches_float64(c):
    _lib, L = _api()
    b, t = 3, 7
    rows = b * t
    x = 2.0 * torch.randn(rows, 2 * c, generator=torch.Generator().manual_seed(c))
    ref = x[:, :c].double() * torch.sigmoid(x[:, c:].double())
    dx = x.cuda()
    y0, y1, y16 = _nan(rows, c), _nan(rows, c), _nan(rows, c, dtype=BF)
    assert L.ts_w2v_glu_fwd(dx.data_ptr(), rows, c, y0.data_ptr(), None, _stream()) == 0
    assert L.ts_w2v_glu_fwd(dx.data_ptr(), rows, c, y1.data_ptr(), y16.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    _assert_close(y0, ref, 1e-5, f"glu c={c}")
    assert torch.equal(y0, y1) and torch.equal(y16.view(torch.int16), y1.to(BF).view(torch.int16))


# ---------------------------------------------------------------------------------------------------------------------
# 3. conv layer 0 and the conv layers behind it
# ---------------------------------------------------------------------------------------------------------------------
CONV0_FRAMES = [1, 7, 8, 9, 255, 256, 257, 1300]     # around the 8-frame unrolled block and the 256-frame chunk; 1300: GroupNorm statistics over six chunks


@pytest.mark.parametrize("c", [1, 31, 32, 130, 512, 514, 640])               # odd: the single-element tail store; above 512: a second trip of the channel loop
@pytest.mark.parametrize("kernel,stride", [(10, 5), (10, 4), (3, 2), (16, 5), (1, 1), (7, 7)])      # (10, 5) has an instantiation of its own
def test_conv_layer_0_matches_float64(kernel, stride, c):
    """conv1d -> GroupNorm(c, c) -> erf-GELU (gn_w given) and conv1d (+ bias) (gn_w NULL); three clips with their own DC offset and gain, so a statistic
    taken over the wrong clip lands far away.  The offsets stay below one spread of the signal, as behind the waveform normaliser.  One frame is the
    degenerate GroupNorm: the value is its own mean and the result is gelu(beta) whatever the signal (the affine form scale v + shift was up to 1.7e-4 off
    there, 400 x the bound, until the finalize kernel learnt the case)."""
    _lib, L = _api()
    b = 3
    gain, offset = torch.tensor([1.0, 0.5, 2.0]), torch.tensor([0.0, 0.3, -0.5])
    g = torch.Generator().manual_seed(100 * kernel + stride + c)
    w = torch.randn(c, kernel, generator=g) / math.sqrt(kernel)
    gn_w, gn_b = 1.0 + 0.3 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g)
    dw, dgw, dgb = w.cuda(), gn_w.cuda(), gn_b.cuda()
    for frames in CONV0_FRAMES:
        n = (frames - 1) * stride + kernel + (stride - 1 if frames % 2 else 0)       # trailing samples that start no frame
        wave = gain[:, None] * torch.randn(b, n, generator=g) + offset[:, None]
        conv = F.conv1d(wave.double()[:, None, :], w.double()[:, None, :], stride=stride)            # [b][c][frames]
        assert conv.shape[2] == frames
        dwave = wave.cuda()
        ws = _ws(L.ts_w2v_conv0_workspace_bytes(b, n, c, kernel, stride))
        refs = {"group": _gelu64(F.group_norm(conv, c, gn_w.double(), gn_b.double(), eps=1e-5)), "bias": conv + gn_b.double()[None, :, None], "plain": conv}
        for mode, ref in refs.items():
            ref = ref.transpose(1, 2).reshape(-1)
            numel = b * frames * c
            outs = {}
            for form in ("y", "y16", "both"):
                y = _nan(numel + 4) if form != "y16" else None                  # four sentinels behind the last row
                y16 = _nan(numel + 4, dtype=BF) if form != "y" else None
                ws.fill_(0xFF)
                st = L.ts_w2v_conv0_fwd(dwave.data_ptr(), b, n, dw.data_ptr(), dgw.data_ptr() if mode == "group" else None,
                                        None if mode == "plain" else dgb.data_ptr(), c, kernel, stride, 1e-5, _ptr(y), _ptr(y16), ws.data_ptr(), _stream())
                assert st == 0
                outs[form] = (y, y16)
            torch.cuda.synchronize()
            what = f"conv0 k={kernel} s={stride} c={c} frames={frames} {mode}"
            y = outs["y"][0]
            _assert_close(y[:numel], ref, 1e-5, what)
            assert torch.equal(outs["both"][0][:numel], y[:numel]), what
            for form in ("y16", "both"):
                assert torch.equal(outs[form][1][:numel].view(torch.int16), y[:numel].to(BF).view(torch.int16)), what + f": y_bf16 ({form})"
            for yy, yy16 in outs.values():
                assert (yy is None or bool(torch.isnan(yy[numel:]).all())) and (yy16 is None or bool(torch.isnan(yy16[numel:]).all())), what + ": written behind the end"


def test_conv_layer_0_refuses_a_kernel_above_sixteen():
    _lib, L = _api()
    wave, w, y = torch.zeros(1, 400, device="cuda"), torch.zeros(8, 17, device="cuda"), torch.zeros(400 * 8, device="cuda")
    ws = _ws(L.ts_w2v_conv0_workspace_bytes(1, 400, 8, 17, 5))
    call = lambda k: L.ts_w2v_conv0_fwd(wave.data_ptr(), 1, 400, w.data_ptr(), None, None, 8, k, 5, 1e-5, y.data_ptr(), None, ws.data_ptr(), _stream())
    assert call(17) == _lib.TS_EUNSUPPORTED and call(16) == 0
    torch.cuda.synchronize()


CONV_KS = [(3, 2), (2, 2), (3, 1), (5, 2)]           # the f32 tap loop goes `stride` taps at a time: 2 + 1, 2, 1 + 1 + 1, 2 + 2 + 1


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("kernel,stride", CONV_KS)
def test_conv_layers_match_float64(kernel, stride, precision):
    _lib, L = _api()
    b, t_in = 3, 41
    c_in, c_out = (32, 64) if precision else (24, 36)                        # bf16: the shapes ts_gemm_nt_bf16 takes (n, k multiples of 32)
    t_out = (t_in - kernel) // stride + 1
    g = torch.Generator().manual_seed(10 * kernel + stride + precision)
    dt = BF if precision else torch.float32
    x = (torch.randn(b, t_in, c_in, generator=g) + torch.arange(b, dtype=torch.float32)[:, None, None]).to(dt)
    w = (torch.randn(c_out, c_in, kernel, generator=g) / math.sqrt(c_in * kernel)).to(dt)
    bias = 0.5 * torch.randn(c_out, generator=g)
    conv = F.conv1d(x.double().transpose(1, 2), w.double(), stride=stride).transpose(1, 2)          # [b][t_out][c_out]
    assert conv.shape[1] == t_out
    dx, dw_, db = x.cuda(), w.permute(0, 2, 1).contiguous().cuda(), bias.cuda()                    # w_taps [c_out][kernel][c_in]
    for use_bias in (False, True):
        for act in (0, 1):
            ref = conv + (bias.double() if use_bias else 0.0)
            ref = _gelu64(ref) if act else ref
            what = f"conv k={kernel} s={stride} precision={precision} bias={use_bias} act={act}"
            call = lambda y, y16: L.ts_w2v_conv_fwd(dx.data_ptr(), b, t_in, c_in, dw_.data_ptr(), db.data_ptr() if use_bias else None, c_out, kernel, stride, act,
                                                    precision, y.data_ptr(), _ptr(y16), None, _stream())
            y, acc, y16 = _nan(b, t_out, c_out), _nan(b, t_out, c_out), _nan(b, t_out, c_out, dtype=BF)
            assert call(y, None) == 0 and call(acc, y16) == 0               # with y_bf16 the f32 buffer is only the accumulator
            torch.cuda.synchronize()
            if precision:
                _assert_bf16_product(y, ref, what)
                _assert_bf16_product(y16, ref, what + " y_bf16")
            else:
                _assert_close(y, ref, 2e-6 * math.sqrt(kernel * c_in) + 1e-5, what, extra=1e-6)
                assert torch.equal(y16.view(torch.int16), y.to(BF).view(torch.int16)), what + ": y_bf16 is not the rounding of y"


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("groups", [1, 4])
@pytest.mark.parametrize("kernel", [5, 4])
def test_grouped_conv_matches_float64(kernel, groups, precision):
    """A layer of data2vec-audio's positional convs: grouped conv1d with padding kernel / 2, the last frame of an even kernel dropped, + bias."""
    _lib, L = _api()
    b, t, c = 3, 50, 64
    cg = c // groups
    g = torch.Generator().manual_seed(10 * kernel + groups + precision)
    x = torch.randn(b, t, c, generator=g) + torch.arange(b, dtype=torch.float32)[:, None, None]
    w = torch.randn(c, cg, kernel, generator=g) / math.sqrt(cg * kernel)
    bias = 0.5 * torch.randn(c, generator=g)
    if precision:                                                            # the kernel rounds x itself: give it values bf16 holds exactly
        x, w = x.to(BF).float(), w.to(BF)
    ref = F.conv1d(x.double().transpose(1, 2), w.double(), bias.double(), padding=kernel // 2, groups=groups)[..., :t].transpose(1, 2)
    w_taps = w.view(groups, cg, cg, kernel).permute(3, 0, 1, 2).contiguous().cuda()          # [kernel][groups][out][in]
    dx, db = x.cuda(), bias.cuda()
    ws = _ws(L.ts_w2v_posconv_workspace_bytes(b, t, c, kernel))
    ws.fill_(0xFF)
    y = _nan(b, t, c)
    assert L.ts_w2v_groupconv_fwd(dx.data_ptr(), b, t, c, w_taps.data_ptr(), db.data_ptr(), kernel, groups, precision, y.data_ptr(), ws.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    what = f"groupconv k={kernel} groups={groups} precision={precision}"
    if precision:
        _assert_bf16_product(y, ref, what)
    else:
        _assert_close(y, ref, 2e-6 * math.sqrt(kernel * cg) + 1e-5, what, extra=1e-6)


# ---------------------------------------------------------------------------------------------------------------------
# 4. attention
# ---------------------------------------------------------------------------------------------------------------------
def _heads(z, heads):
    b, t, c = z.shape
    return z.reshape(b, t, heads, c // heads).transpose(1, 2)


def _attention_ref(qkv, heads, n):
    """float64 softmax(q k^T / sqrt(hd)) v over the first n[b] keys; over all t keys for n <= 0 (what both inference kernels and transformers do)."""
    b, t, c3 = qkv.shape
    c = c3 // 3
    q, k, v = [_heads(z, heads) for z in qkv.double().split(c, dim=-1)]
    s = (q @ k.transpose(-1, -2)) / math.sqrt(c // heads)
    lim = torch.where(n > 0, n, torch.full_like(n, t))
    s = s.masked_fill((torch.arange(t)[None, :] >= lim[:, None])[:, None, None, :], float("-inf"))
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(b, t, c)


@pytest.mark.parametrize("t", [1, 7, 31, 32, 33, 64, 128, 129, 500])
@pytest.mark.parametrize("precision,hd", [(0, 64), (1, 64), (0, 16), (1, 16), (0, 80), (1, 80)])       # bf16 with head_dim 64: the fused kernel; else materialised
def test_inference_attention_matches_float64(precision, hd, t):
    _lib, L = _api()
    heads = 2
    c = heads * hd
    lens = [0, 1, 31, 32, 33, 63, 64, 65, t, t + 5]                          # one clip each; a length above t counts as t
    for key_len in (torch.tensor(lens, dtype=torch.int32), None):
        b = len(lens) if key_len is not None else 2
        g = torch.Generator().manual_seed(1000 * precision + 10 * t + hd + b)
        qkv = (1.5 * torch.randn(b, t, 3 * c, generator=g)).to(BF if precision else torch.float32)
        n = key_len.long().clamp(max=t) if key_len is not None else torch.full((b,), t)
        ref = _attention_ref(qkv, heads, n)
        dq, kl = qkv.cuda(), (key_len.cuda() if key_len is not None else None)
        ctx = _nan(b, t, c, dtype=qkv.dtype)
        ws = _ws(L.ts_w2v_attention_workspace_bytes(b, t, heads, precision))
        assert L.ts_w2v_attention_fwd(dq.data_ptr(), b, t, c, heads, _ptr(kl), precision, ctx.data_ptr(), ws.data_ptr(), _stream()) == 0
        torch.cuda.synchronize()
        what = f"attention precision={precision} hd={hd} t={t} key_len={'ragged' if key_len is not None else 'NULL'}"
        if precision:
            _assert_bf16_product(ctx, ref, what)
        else:
            _assert_close(ctx, ref, 2e-6 * math.sqrt(t) + 1e-5, what, extra=1e-6)


# ---- fused training attention ---------------------------------------------------------------------------------------
# (b, t, heads, p, key_len).  Ragged clips hold t, 0 and one of 1, 63, 64, 65; a two-clip batch has room for two of the three, so 0 sits in the
# three-clip cases and the two-clip ones pair a full clip with a short one.
TRAIN_CASES = [(2, 1, 1, 0.0, None), (2, 31, 1, 0.1, (31, 1)), (2, 64, 2, 0.0, None), (3, 128, 1, 0.1, (128, 0, 63)), (3, 129, 2, 0.0, (129, 0, 65)),
               (2, 499, 2, 0.1, (499, 64)), (1, 999, 1, 0.0, None), (2, 999, 1, 0.1, (999, 65))]
TRAIN_SEED = 20240917
LN2 = math.log(2.0)


def _bf(x):
    return x.float().to(BF).double()


def _train_inputs(b, t, heads):
    # A block of ONE row (t = 129: row 128) whose softmax is nearly one-hot has dS = P (dP - D) near 0, and its relative error then measures the conditioning
    # of that row, not the arithmetic: with the generator seeded 1000 b + t + heads the bf16-rounding emulation itself is 8.5e-2 off float64 on that block
    # (dq row norm 0.41 against about 5 elsewhere).  The seed below is the next one; it was chosen by the CPU emulation alone (seeds + 0 .. + 7 give a worst
    # emulated block of 8.5e-2, 8.6e-3, 1.4e-2, 1.3e-2, 2.9e-2, 6.4e-3, 5.6e-3, 1.4e-2), and the test asserts that the emulation stays under a third of the cap.
    g = torch.Generator().manual_seed(1000 * b + t + heads + 1)
    c = 64 * heads
    return (1.5 * torch.randn(b, t, 3 * c, generator=g)).to(BF), torch.randn(b, t, c, generator=g)


def _train_keep(b, heads, t, p):
    """ts_train_dropout's keep decisions over the logical [B H t][t] matrix (ones in, kept elements nonzero out)."""
    _lib, L = _api()
    ones = torch.ones(b * heads * t, t, device="cuda")
    out = _nan(b * heads * t, t)
    assert L.ts_train_dropout(ones.data_ptr(), out.data_ptr(), b * heads * t, t, t, float(p), TRAIN_SEED, None, 0, _stream()) == 0
    torch.cuda.synchronize()
    return (out != 0).view(b, heads, t, t).cpu()


def _valid_keys(key_len, b, t):
    return torch.full((b,), t) if key_len is None else torch.tensor(key_len).long().clamp(max=t)


def _train_scores(q16, heads, n, dtype=torch.float64):
    b, t, c3 = q16.shape
    q, k, v = [_heads(z, heads) for z in q16.to(dtype).split(c3 // 3, dim=-1)]
    s = (q @ k.transpose(-1, -2)) / 8.0
    return q, k, v, s.masked_fill((torch.arange(t)[None, :] >= n[:, None])[:, None, None, :], float("-inf"))


def _train_reference(q16, n, heads, p, keep, dout):
    """float64 autograd of dropout(softmax(q k^T / 8 + key mask)) v on the bf16-rounded q / k / v; a clip without a valid key has probability 0 everywhere.
    Returns ctx, dqkv and lse2 = log2(sum over the valid keys of exp(s / 8))."""
    b, t, c3 = q16.shape
    c = c3 // 3
    qkv = q16.double().requires_grad_(True)
    q, k, v = [_heads(z, heads) for z in qkv.split(c, dim=-1)]
    s = (q @ k.transpose(-1, -2)) / 8.0
    pad = torch.arange(t)[None, :] >= n[:, None]
    s = s.masked_fill((pad & (n[:, None] > 0))[:, None, None, :], float("-inf"))
    prob = torch.softmax(s, -1) * (n > 0).double()[:, None, None, None]
    if p > 0:
        prob = prob * keep.double() / (1.0 - p)
    ctx = (prob @ v).transpose(1, 2).reshape(b, t, c)
    ctx.backward(dout.double())
    return ctx.detach(), qkv.grad, torch.logsumexp(s.detach(), -1) / LN2


def _train_emulation(q16, n, heads, p, keep, dout, rnd):
    """The same mathematics written out, with `rnd` applied where the kernels hold bf16 (csrc/w2v_attn_train.hip's header): P keep / (1 - p) before P V,
    dO, dS; everything else float64.  With rnd = identity it is the reference (asserted below), with rnd = bf16 rounding it is the reference's own error
    under the kernels' operand precision."""
    b, t, c3 = q16.shape
    c = c3 // 3
    q, k, v, s = _train_scores(q16, heads, n)
    prob = torch.nan_to_num(torch.softmax(s, -1), nan=0.0)                   # a clip without a valid key: all -inf -> NaN -> 0
    kp = keep.double() / (1.0 - p) if p > 0 else 1.0
    pd = rnd(prob * kp)
    ctx = pd @ v
    do = _heads(dout.double(), heads)
    d = (do * ctx).sum(-1, keepdim=True)
    do_r = rnd(do)
    ds = rnd(prob * ((do_r @ v.transpose(-1, -2)) * kp - d))
    flat = lambda z: z.transpose(1, 2).reshape(b, t, c)
    return flat(ctx), torch.cat([flat(ds @ k / 8.0), flat(ds.transpose(-1, -2) @ q / 8.0), flat(pd.transpose(-1, -2) @ do_r)], -1)


def _block_norms(x, heads):
    """[b][t][64 heads] -> L2 norm per (clip, block of 32 time rows, head): the unit one wave owns"""
    b, t, c = x.shape
    nb = (t + 31) // 32
    z = torch.zeros(b, nb * 32, c, dtype=torch.float64)
    z[:, :t] = x.double()
    return z.view(b, nb, 32, heads, 64).pow(2).sum(dim=(2, 4)).sqrt()


def _block_classes(name, n, t, heads):
    """Class of every block [b][nb][heads], from the reference alone: 1 structurally zero, 2 zero in exact arithmetic only, 3 the rest."""
    b, nb = n.shape[0], (t + 31) // 32
    cls = torch.full((b, nb, heads), 3)
    if name in ("dq", "dk"):
        cls[n == 1] = 2                                                       # one key per row: dS = P (dP - D) = 0
    if name in ("dk", "dv"):
        first = 32 * torch.arange(nb)
        cls[(first[None, :] >= n[:, None])[:, :, None].expand(b, nb, heads)] = 1      # every row of the block is a key >= key_len
    cls[n <= 0] = 1
    return cls


def _split_outputs(ctx, dqkv):
    c = ctx.shape[-1]
    return {"ctx": ctx, "dq": dqkv[..., :c], "dk": dqkv[..., c:2 * c], "dv": dqkv[..., 2 * c:]}


@functools.lru_cache(maxsize=None)
def _emulated_block_error():
    """Largest class-3 block error, and largest whole-tensor error, of the bf16-rounding emulation against pure float64 over TRAIN_CASES."""
    worst_block, worst_whole = 0.0, 0.0
    for b, t, heads, p, key_len in TRAIN_CASES:
        q16, dout = _train_inputs(b, t, heads)
        n = _valid_keys(key_len, b, t)
        keep = _train_keep(b, heads, t, p) if p > 0 else None
        rctx, rdqkv, _ = _train_reference(q16, n, heads, p, keep, dout)
        exact = _train_emulation(q16, n, heads, p, keep, dout, lambda z: z)
        assert float((exact[0] - rctx).abs().max()) <= 1e-9 and float((exact[1] - rdqkv).abs().max()) <= 1e-9      # the emulation restates the reference
        emu = _split_outputs(*_train_emulation(q16, n, heads, p, keep, dout, _bf))
        for name, ref in _split_outputs(rctx, rdqkv).items():
            cls = _block_classes(name, n, t, heads)
            err, size = _block_norms(emu[name] - ref, heads), _block_norms(ref, heads)
            if bool((cls == 3).any()):
                worst_block = max(worst_block, float((err[cls == 3] / size[cls == 3]).max()))
            if float(ref.norm()) > 1e-6 * float(rctx.norm()):
                worst_whole = max(worst_whole, float((emu[name] - ref).norm() / ref.norm()))
    return worst_block, worst_whole


@pytest.mark.parametrize("b,t,heads,p,key_len", TRAIN_CASES)
def test_fused_training_attention_matches_float64_block_by_block(b, t, heads, p, key_len):
    """ts_w2v_attention_train_fwd / _bwd: ctx, dq, dk, dv and lse2 against float64 autograd, the dropout mask taken from ts_train_dropout.

    Whole tensors: 2e-2 relative L2.  Per block of 32 time rows x one head (no block left out): class 1 (clip without a valid key; dk / dv rows all at
    keys >= key_len) exactly zero; class 2 (one key per row: dq, dk vanish in exact arithmetic, the kernel holds the bf16 rounding of dP against the f32 D)
    at most 2e-2 of the norm of the clip's dv; class 3 within 3 x the largest class-3 block error of the bf16-rounding emulation over all cases, capped
    at 5e-2.  lse2 = log2(sum over the valid keys of exp(s / 8)) within 4 x the error of the same expression in float32 on the CPU, floor 1e-5 x max |lse2|;
    for a clip without a valid key the kernel stores +inf there (every rebuilt probability exp2(s - inf) is 0), which is asserted instead.

    Measured.  Emulation against float64 on these inputs: whole tensors 1.6e-3 .. 7.6e-3, worst class-3 block 8.6e-3 (dq, t = 129, the one-row block of the
    clip with key_len 65), so the block bound is 2.6e-2.  Kernels on an MI355X: whole tensors 6.9e-4 .. 7.3e-3; worst class-3 block per case 1.9e-3 (t = 1),
    3.3e-3, 4.2e-3, 3.4e-3, 1.3e-2 (t = 129, the same one-row block), 4.8e-3, 3.9e-3, 5.2e-3; class 2 at most 3.5e-3 of the clip's dv; lse2 off by
    7.8e-7 .. 1.6e-6 against 8.1e-7 .. 2.3e-6 for float32 on the CPU (bounds 1.1e-4 .. 1.8e-4: the floor binds)."""
    _lib, L = _api()
    c = 64 * heads
    q16, dout = _train_inputs(b, t, heads)
    n = _valid_keys(key_len, b, t)
    keep = _train_keep(b, heads, t, p) if p > 0 else None
    dq16, ddout = q16.cuda(), dout.cuda()
    kl = torch.tensor(key_len, dtype=torch.int32).cuda() if key_len is not None else None
    ctx, lse2, dqkv = _nan(b, t, c), _nan(b, heads, t), _nan(b, t, 3 * c)
    wsf = _ws(L.ts_w2v_attention_train_fwd_workspace(b, t, c, heads))
    assert L.ts_w2v_attention_train_fwd(dq16.data_ptr(), b, t, c, heads, _ptr(kl), p, TRAIN_SEED, ctx.data_ptr(), lse2.data_ptr(), wsf.data_ptr(), _stream()) == 0
    wsb = _ws(L.ts_w2v_attention_train_bwd_workspace(b, t, c, heads))
    assert L.ts_w2v_attention_train_bwd(dq16.data_ptr(), b, t, c, heads, _ptr(kl), p, TRAIN_SEED, ddout.data_ptr(), ctx.data_ptr(), lse2.data_ptr(), None,
                                        dqkv.data_ptr(), wsb.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    ctx, lse2, dqkv = ctx.cpu(), lse2.cpu(), dqkv.cpu()
    assert bool(torch.isfinite(ctx).all()) and bool(torch.isfinite(dqkv).all()) and not bool(torch.isnan(lse2).any())
    rctx, rdqkv, rlse2 = _train_reference(q16, n, heads, p, keep, dout)
    got, ref = _split_outputs(ctx, dqkv), _split_outputs(rctx, rdqkv)

    # the row statistic
    some = n > 0
    assert bool((lse2[~some] == float("inf")).all())
    if bool(some.any()):
        lse32 = torch.logsumexp(_train_scores(q16, heads, n, torch.float32)[3], -1) / LN2
        own = float((lse32.double() - rlse2)[some].abs().max())
        bound = max(4.0 * own, 1e-5 * float(rlse2[some].abs().max()))
        err = float((lse2.double() - rlse2)[some].abs().max())
        print(f"lse2 b={b} t={t}: error {err:.3e}, float32 on the CPU {own:.3e}, bound {bound:.3e}")
        assert err <= bound, (err, bound)

    # structural zeros, row by row
    for i in range(b):
        ni = int(n[i])
        assert float(got["dk"][i, max(ni, 0):].abs().max() if ni < t else 0.0) == 0.0 and float(got["dv"][i, max(ni, 0):].abs().max() if ni < t else 0.0) == 0.0
        if ni <= 0:
            assert all(float(z[i].abs().max()) == 0.0 for z in got.values())

    worst_block, worst_whole = _emulated_block_error()
    assert 3.0 * worst_block <= 5e-2, "the inputs are ill-conditioned for a per-block relative error: the reference's own bf16 emulation is beyond the cap"
    block_bound = min(3.0 * worst_block, 5e-2)
    print(f"emulation: worst class-3 block {worst_block:.3e}, worst whole tensor {worst_whole:.3e}; block bound {block_bound:.3e}")
    dv_clip = ref["dv"].reshape(b, -1).norm(dim=1)
    for name in ("ctx", "dq", "dk", "dv"):
        g_, r_ = got[name], ref[name]
        if float(r_.norm()) > 1e-6 * float(rctx.norm()):
            whole = float((g_.double() - r_).norm() / r_.norm())
            assert whole <= 2e-2, (name, whole)
        else:
            whole = float(g_.double().norm() / ref["dv"].norm())
            assert whole <= 2e-2, (name, whole)
        cls = _block_classes(name, n, t, heads)
        size_got, size_ref, err = _block_norms(g_, heads), _block_norms(r_, heads), _block_norms(g_.double() - r_, heads)
        assert bool((size_got[cls == 1] == 0).all()), name + ": a structurally zero block is not zero"
        two = cls == 2
        if bool(two.any()):
            assert bool((size_got <= 2e-2 * dv_clip[:, None, None])[two].all()), (name, float((size_got / dv_clip[:, None, None])[two].max()))
        three = cls == 3
        worst = float((err[three] / size_ref[three]).max()) if bool(three.any()) else 0.0
        print(f"{name} b={b} t={t} heads={heads} p={p}: whole {whole:.3e}; blocks: {int((cls == 1).sum())} zero, {int(two.sum())} vanishing, "
              f"{int(three.sum())} compared, worst {worst:.3e}")
        assert worst <= block_bound, (name, worst, block_bound)
