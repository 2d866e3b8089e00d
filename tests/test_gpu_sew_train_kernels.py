"""GPU parity of the three launches of csrc/sew_train.hip (through include/thunder_speech_amd/sew_train.h) against float64 on the CPU, element by
element: the training forward of SEW's squeeze (y bit-equal to the inference call's, z the conv result), its data gradient and its weight gradient.
Every output starts as NaN, every workspace as 0xFF bytes, every return code is asserted.  The references read what the kernels read: bf16-rounded
conv operands (x, dz, w) and the f32 pool operand; the bound is the matrix-core bound of tests/test_gpu_sew.py, max 0.03 and rms 0.006 of
max |reference|.  Shapes (its _squeeze_case and _frames): B = 2 with different data per clip, 32 and 24 channels per group, 15 / 16 / 128 taps,
T in {s, 7, 261, 2 x 128 + 2 s + 1, s x 128 + 2 s + 1} -- a single output frame, ragged tails, T % s != 0 behind one and behind s tiles of 128 frames.
Measured on an MI355X: with the operands rounded alike on both sides only the f32 accumulation order is left -- max error below 1e-6 of
max |reference| in z, dx and dw on the shapes looked at, against the 3e-2 allowed."""
import functools

import pytest
import torch
import torch.nn.functional as F

transformers = pytest.importorskip("transformers")

pytestmark = pytest.mark.gpu

from test_gpu_sew import B, BF, GEOMETRIES, _api, _frames, _nan, _squeeze_case, _stream, _ws       # noqa: E402  (the shapes, the data and the NaN / 0xFF helpers)

TRAIN_GEOMETRIES = ["c128_g4", "c192_g8"]                      # 32 and 24 channels per group: the widths that train


@functools.lru_cache(maxsize=None)
def _train_case(geometry, k, s, t, zero_tail=False):
    """(x, w, bias, dz, dy, float64 references z, dx, dx's conv term, dw) of one shape; computed once.  dz, dy [B][T // s][C]."""
    c, groups = GEOMETRIES[geometry]
    cg = c // groups
    x, w, bias, _, _ = _squeeze_case(geometry, k, s, t, zero_tail)
    t2 = t // s
    g = torch.Generator().manual_seed(7 + 100000 * c + 1000 * k + 10 * t + s)
    dz = torch.randn(B, t2, c, generator=g) * (1.0 + 0.5 * torch.arange(B, dtype=torch.float32)[:, None, None])
    dy = torch.randn(B, t2, c, generator=g)
    if zero_tail:
        dz[1, 2 * t2 // 3:] = 0.0
        dy[1, 2 * t2 // 3:] = 0.0
    x16, w16, dz16 = x.to(BF).double().transpose(1, 2), w.to(BF).double(), dz.to(BF).double().transpose(1, 2)
    p = k // 2
    full = F.conv1d(x16, w16, None, stride=s, padding=p, groups=groups)
    n_out = full.shape[-1]
    assert n_out >= t2
    z = full[..., :t2].transpose(1, 2).contiguous()
    dzf = F.pad(dz16, (0, n_out - t2))                          # the conv frames transformers trims get no gradient
    conv_t = torch.nn.grad.conv1d_input((B, c, t), w16, dzf, stride=s, padding=p, groups=groups).transpose(1, 2).contiguous()
    pool_t = torch.zeros(B, t, c, dtype=torch.float64)
    pool_t[:, :s * t2] = dy.double().repeat_interleave(s, dim=1) / s
    dw = torch.nn.grad.conv1d_weight(x16, (c, cg, k), dzf, stride=s, padding=p, groups=groups)
    dw = dw.view(groups, cg, cg, k).permute(3, 0, 1, 2).contiguous()
    return x, w, bias, dz, dy, z, conv_t + pool_t, conv_t, dw


def _calls(geometry, k, s, t, zero_tail=False, dy_override=None):
    """One call of each launch on the case's data -> (status, {y, z, dx, dw, y_inference}); refused geometries leave every output NaN."""
    from thunder_speech_amd.huggingface.sew import pack_squeeze_taps
    from thunder_speech_amd.huggingface.sew_train import pack_squeeze_dgrad_taps, squeeze_trains
    _lib, L = _api()
    c, groups = GEOMETRIES[geometry]
    cg = c // groups
    x, w, bias, dz, dy, *_ = _train_case(geometry, k, s, t, zero_tail)
    if dy_override is not None:
        dy = dy_override
    t2 = t // s
    taps = pack_squeeze_taps(w.cuda(), groups, True)
    wk = w.view(groups, cg, cg, k).permute(3, 0, 1, 2).contiguous().cuda()
    dtaps = pack_squeeze_dgrad_taps(wk, s)
    xs, bs, dzs, dys = x.cuda(), bias.cuda(), dz.cuda(), dy.cuda()
    out = dict(y=_nan(B, t2, c), z=_nan(B, t2, c), dx=_nan(B, t, c), dw=_nan(k, groups, cg, cg), y_inference=_nan(B, t2, c))
    st_inf = L.ts_sew_squeeze_fwd(xs.data_ptr(), B, t, c, taps.data_ptr(), bs.data_ptr(), k, groups, s, 1, out["y_inference"].data_ptr(),
                                  _ws(L.ts_sew_squeeze_workspace_bytes(B, t, c, k, s, 1)).data_ptr(), _stream())
    st = [L.ts_sew_squeeze_train_fwd(xs.data_ptr(), B, t, c, taps.data_ptr(), bs.data_ptr(), k, groups, s, out["y"].data_ptr(), out["z"].data_ptr(),
                                     _ws(L.ts_sew_squeeze_workspace_bytes(B, t, c, k, s, 1)).data_ptr(), _stream()),
          L.ts_sew_squeeze_dgrad(dzs.data_ptr(), dys.data_ptr(), B, t, c, dtaps.data_ptr(), k, groups, s, out["dx"].data_ptr(),
                                 _ws(L.ts_sew_squeeze_dgrad_workspace_bytes(B, t, c, k, s)).data_ptr(), _stream()),
          L.ts_sew_squeeze_wgrad(dzs.data_ptr(), xs.data_ptr(), B, t, c, k, groups, s, out["dw"].data_ptr(),
                                 _ws(L.ts_sew_squeeze_wgrad_workspace_bytes(B, t, c, k, s)).data_ptr(), _stream())]
    torch.cuda.synchronize()
    if not squeeze_trains(cg, k, s):
        assert st == [_lib.TS_EUNSUPPORTED] * 3 and st_inf == _lib.TS_EUNSUPPORTED
        assert all(bool(torch.isnan(v).all()) for v in out.values())
        return _lib.TS_EUNSUPPORTED, None
    assert st == [0, 0, 0] and st_inf == 0
    return 0, out


def _assert_close(got, ref, what):
    got = got.double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert not bool(torch.isnan(got).any()), f"{what}: unwritten (NaN) elements"
    scale = float(ref.abs().max())
    mx, rms = float((got - ref).abs().max()), float((got - ref).pow(2).mean().sqrt())
    print(f"{what}: max {mx:.3e} rms {rms:.3e} of scale {scale:.3e}")
    assert mx <= 0.03 * scale and rms <= 0.006 * scale, f"{what}: max {mx:.3e} rms {rms:.3e} against scale {scale:.3e}"


def _check(geometry, k, s, t, zero_tail=False):
    _, _, _, _, _, z, dx, _, dw = _train_case(geometry, k, s, t, zero_tail)
    st, out = _calls(geometry, k, s, t, zero_tail)
    if out is None:
        return False
    what = f"{geometry} k={k} s={s} t={t}" + (" zero tail" if zero_tail else "")
    assert not bool(torch.isnan(out["y"]).any()) and torch.equal(out["y"], out["y_inference"]), f"{what}: y differs from ts_sew_squeeze_fwd's"
    _assert_close(out["z"], z, "z " + what)
    _assert_close(out["dx"], dx, "dx " + what)
    _assert_close(out["dw"], dw, "dw " + what)                     # (24 channels per group: the reference has width 24, no padded lane in it)
    return True


@pytest.mark.parametrize("s", [2, 3])
@pytest.mark.parametrize("k", [15, 16, 128])
@pytest.mark.parametrize("geometry", TRAIN_GEOMETRIES)
def test_forward_dgrad_and_wgrad_match_float64(geometry, k, s):
    ran = [_check(geometry, k, s, t) for t in _frames(s)]
    assert all(ran) is not (k == 128 and s == 3) and len(set(ran)) == 1       # s = 3 with 128 taps: TS_EUNSUPPORTED, outputs still NaN


@pytest.mark.parametrize("geometry", TRAIN_GEOMETRIES)
def test_stride_one(geometry):
    """s = 1: the pool is the identity and the launches are wav2vec2's positional conv at 24 / 32 channels per group."""
    for t in _frames(1):
        assert _check(geometry, 16, 1, t)


@pytest.mark.parametrize("geometry", TRAIN_GEOMETRIES)
def test_a_zero_tailed_clip(geometry):
    """Clip 1's rows from two thirds on are zero in x (ts_w2v_mask_rows) and in the incoming gradients (MaskRows' backward)."""
    for s, k in [(2, 16), (3, 15)]:
        assert _check(geometry, k, s, 261, True)


@pytest.mark.parametrize("geometry", TRAIN_GEOMETRIES)
def test_two_calls_give_equal_bits(geometry):
    for s, k, t in [(2, 128, 261), (3, 15, 391)]:
        (_, a), (_, b) = _calls(geometry, k, s, t), _calls(geometry, k, s, t)
        for name in ("y", "z", "dx", "dw"):
            assert not bool(torch.isnan(a[name]).any()) and torch.equal(a[name], b[name]), (name, s, k, t)


@pytest.mark.parametrize("s,k,t", [(2, 16, 261), (3, 15, 392), (3, 16, 7)])            # T - s T2 = 1, 2, 1
@pytest.mark.parametrize("geometry", TRAIN_GEOMETRIES)
def test_rows_behind_the_last_pooled_frame_hold_the_conv_term_only(geometry, s, k, t):
    """Rows s T2 .. T - 1 are in no pooling window: whatever dy is, they hold conv^T(dz) -- equal bits for two different dy, the float64 conv term
    within the bound, and not zero (the taps do reach them)."""
    c, _ = GEOMETRIES[geometry]
    t2 = t // s
    assert s * t2 < t
    conv_t = _train_case(geometry, k, s, t)[7]
    _, a = _calls(geometry, k, s, t)
    _, b = _calls(geometry, k, s, t, dy_override=torch.full((B, t2, c), 3.0))
    tail_a, tail_b = a["dx"][:, s * t2:], b["dx"][:, s * t2:]
    assert torch.equal(tail_a, tail_b) and not torch.equal(a["dx"][:, :s * t2], b["dx"][:, :s * t2])
    assert float(tail_a.abs().max()) > 0
    err = float((tail_a.double().cpu() - conv_t[:, s * t2:]).abs().max())
    assert err <= 0.03 * float(conv_t.abs().max()), err


@pytest.mark.parametrize("s,rest", [(2, 1), (3, 1), (3, 2)])
def test_the_padding_node_is_exact_forward_and_backward(s, rest):
    from thunder_speech_amd.huggingface.sew_train import UnsqueezeRows
    c, t2 = 128, 87
    t = s * t2 + rest
    g = torch.Generator().manual_seed(10 * s + rest)
    up = torch.randn(B, t2, s * c, generator=g).cuda().requires_grad_(True)
    grad = torch.randn(B, t, c, generator=g).cuda()
    out = UnsqueezeRows.apply(up, t, s)
    assert torch.equal(out[:, :s * t2], up.detach().view(B, s * t2, c)) and not bool(out[:, s * t2:].any())
    out.backward(grad)
    assert torch.equal(up.grad, grad[:, :s * t2].reshape(B, t2, s * c))
