"""The launches behind one layer of data2vec-audio's positional stack in training (csrc/posconv_stack_train.hip and the raw-accumulator epilogue of
w2v_posconv_mfma_kernel in csrc/w2v_posconv.hip, through include/thunder_speech_amd/posconv_stack_train.h) against float64 on the CPU.  Every output
starts as NaN, every workspace as 0xFF bytes, every return code is asserted.  Bounds: the table of tests/test_gpu_w2v_kernels.py --
  forward row kernel (LayerNorm row + GELU)           1e-5 x max |reference| + 2e-6 (the GELU rule)
  backward row kernel: dz and dbias                   1e-5 x max |reference|, against float64 autograd of gelu(layer_norm(z + b, eps = 1e-5))
  raw-epilogue conv, forward and data gradient        bf16-operand products: max 0.03, rms 0.006 of max |reference| (operands rounded to bf16 first)
and the two calls of the backward row kernel, like the two calls of each existing matrix-core entry, give equal bits."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

NAN = float("nan")
BF = torch.bfloat16
EPS = 1e-5
ROW_C = [4, 64, 260, 768, 1024, 1028, 4096]       # NV = 2 | 4 | 8 | 16; 260 and 1028: one lane of the last register slot
ROW_ROWS = [1, 3, 257, 1001]                        # idle waves; a last workgroup with fewer than its 8 rows; 33 and 126 partial rows of the bias gradient


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _api():
    from thunder_speech_amd import _lib
    return _lib, _lib.lib()


def _nan(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device="cuda")


def _ws(nbytes):
    assert nbytes > 0
    return torch.full((int(nbytes),), 0xFF, dtype=torch.uint8, device="cuda")


def _assert_close(got, ref, rel, what, extra=0.0):
    got = got.detach().double().cpu()
    assert not bool(torch.isnan(got).any()), f"{what}: unwritten (NaN) elements"
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    err, scale = float((got - ref.double()).abs().max()), float(ref.abs().max())
    print(f"{what}: max error {err:.3e}, bound {rel * scale + extra:.3e}")
    assert err <= rel * scale + extra, f"{what}: max error {err:.3e} > {rel:.1e} x {scale:.3e} + {extra:.1e}"


def _assert_bf16_product(got, ref, what):
    got = got.detach().double().cpu()
    assert not bool(torch.isnan(got).any()), f"{what}: unwritten (NaN) elements"
    scale = float(ref.abs().max())
    mx, rms = float((got - ref).abs().max()), float((got - ref).pow(2).mean().sqrt())
    print(f"{what}: max {mx:.3e} rms {rms:.3e} of scale {scale:.3e}")
    assert mx <= 0.03 * scale and rms <= 0.006 * scale, f"{what}: max {mx:.3e} rms {rms:.3e} against scale {scale:.3e}"


# ---------------------------------------------------------------------------------------------------------------------
# 1. the row kernels
# ---------------------------------------------------------------------------------------------------------------------
def _row_case(z, bias, da, what):
    """Forward, backward (twice) of the row kernels on (z [rows][c], bias [c], da [rows][c]) against float64 autograd."""
    _lib, L = _api()
    rows, c = z.shape
    zr = z.double().requires_grad_(True)
    br = bias.double().requires_grad_(True)
    ref = F.gelu(F.layer_norm(zr + br, (c,), eps=EPS))
    ref.backward(da.double())
    dz_, db_, da_ = z.cuda(), bias.cuda(), da.cuda()
    a = _nan(rows, c)
    assert L.ts_posconv_stack_norm_gelu_fwd(dz_.data_ptr(), db_.data_ptr(), EPS, rows, c, a.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    _assert_close(a, ref.detach(), 1e-5, what + " forward", extra=2e-6)
    nbytes = L.ts_posconv_stack_norm_gelu_bwd_workspace(rows, c)
    outs = []
    for _ in range(2):
        ws, dz, dbias = _ws(nbytes), _nan(rows, c), _nan(c)
        assert L.ts_posconv_stack_norm_gelu_bwd(dz_.data_ptr(), db_.data_ptr(), da_.data_ptr(), EPS, rows, c, dz.data_ptr(), dbias.data_ptr(), ws.data_ptr(),
                                                _stream()) == 0
        torch.cuda.synchronize()
        outs.append((dz, dbias))
    _assert_close(outs[0][0], zr.grad, 1e-5, what + " dz")
    _assert_close(outs[0][1], br.grad, 1e-5, what + " dbias")
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), what + ": two calls differ"


@pytest.mark.parametrize("rows", ROW_ROWS)
@pytest.mark.parametrize("c", ROW_C)
def test_row_kernels_match_float64_autograd(c, rows):
    g = torch.Generator().manual_seed(11 * c + rows)
    z = 2.0 * torch.randn(rows, c, generator=g) + 3.0                          # the mean is larger than the spread
    bias = 0.3 * torch.randn(c, generator=g)
    da = torch.randn(rows, c, generator=g)
    _row_case(z, bias, da, f"norm_gelu c={c} rows={rows}")


@pytest.mark.parametrize("c", [768, 1024])
def test_row_kernels_on_a_row_of_variance_zero(c):
    """Row 1 has z + bias = 3 in every channel, exactly (the bias is a multiple of 1 / 64, so z = 3 - bias and the sum are exact in f32 and in float64: the
    reference's row has variance 0 too): n = 0, a = 0, rstd = 1 / sqrt(eps) -- finite, and the float64 values within the same bounds."""
    g = torch.Generator().manual_seed(c)
    z = 2.0 * torch.randn(5, c, generator=g) + 3.0
    bias = torch.round(0.3 * torch.randn(c, generator=g) * 64.0) / 64.0
    z[1] = 3.0 - bias
    assert float((z[1].double() + bias.double()).var()) == 0.0
    da = torch.randn(5, c, generator=g)
    _row_case(z, bias, da, f"norm_gelu variance 0, c={c}")


def test_row_kernels_refuse_widths_and_pointers_they_cannot_vectorise():
    _lib, L = _api()
    rows = 8
    buf = lambda c: torch.zeros(rows * c + 8, device="cuda")
    for c in (6, 4100):
        z, b, a, da, dz, db = (buf(c) for _ in range(6))
        ws = _ws(max(L.ts_posconv_stack_norm_gelu_bwd_workspace(rows, c), 16) + 16)
        assert L.ts_posconv_stack_norm_gelu_fwd(z.data_ptr(), b.data_ptr(), EPS, rows, c, a.data_ptr(), _stream()) == _lib.TS_EUNSUPPORTED
        assert L.ts_posconv_stack_norm_gelu_bwd(z.data_ptr(), b.data_ptr(), da.data_ptr(), EPS, rows, c, dz.data_ptr(), db.data_ptr(), ws.data_ptr(),
                                                _stream()) == _lib.TS_EUNSUPPORTED
    c = 64
    z, b, a, da, dz, db = (buf(c) for _ in range(6))
    ws = _ws(L.ts_posconv_stack_norm_gelu_bwd_workspace(rows, c) + 16)
    fwd = [z.data_ptr(), b.data_ptr(), a.data_ptr()]
    for i in range(3):
        p = list(fwd)
        p[i] += 4
        assert L.ts_posconv_stack_norm_gelu_fwd(p[0], p[1], EPS, rows, c, p[2], _stream()) == _lib.TS_EUNSUPPORTED, i
    bwd = [z.data_ptr(), b.data_ptr(), da.data_ptr(), dz.data_ptr(), db.data_ptr(), ws.data_ptr()]
    for i in range(6):
        p = list(bwd)
        p[i] += 4
        assert L.ts_posconv_stack_norm_gelu_bwd(p[0], p[1], p[2], EPS, rows, c, p[3], p[4], p[5], _stream()) == _lib.TS_EUNSUPPORTED, i
    assert L.ts_posconv_stack_norm_gelu_fwd(None, b.data_ptr(), EPS, rows, c, a.data_ptr(), _stream()) == _lib.TS_EINVAL
    assert L.ts_posconv_stack_norm_gelu_bwd(z.data_ptr(), b.data_ptr(), da.data_ptr(), EPS, 0, c, dz.data_ptr(), db.data_ptr(), ws.data_ptr(), _stream()) == _lib.TS_EINVAL
    assert L.ts_posconv_stack_norm_gelu_bwd_workspace(0, c) == _lib.TS_EINVAL
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the conv with the raw-accumulator epilogue
# ---------------------------------------------------------------------------------------------------------------------
B, G, CG = 2, 2, 64
C = G * CG


@functools.lru_cache(maxsize=None)
def _conv_reference(t, k):
    """bf16-rounded (x, w [C][C / g][k], dz) as float64, conv(x) and the input gradient of <conv(x), dz> by float64 autograd; computed once per shape."""
    g = torch.Generator().manual_seed(1000 * t + k)
    x = torch.randn(B, t, C, generator=g).to(BF)                               # the two clips hold different data
    w = (torch.randn(C, CG, k, generator=g) * (CG * k) ** -0.5).to(BF)
    dz = torch.randn(B, t, C, generator=g).to(BF)
    xr = x.double().requires_grad_(True)
    z = F.conv1d(xr.transpose(1, 2), w.double(), padding=k // 2, groups=G)[..., :t].transpose(1, 2)
    z.backward(dz.double())
    return x, w, dz, z.detach(), xr.grad


def _taps(w, k):
    """conv.weight [C][C / g][k] -> [k][groups][out][in]"""
    return w.view(G, CG, CG, k).permute(3, 0, 1, 2).contiguous()


@pytest.mark.parametrize("k", [19, 8, 2])                                      # odd; even (the dropped last frame); the smallest
@pytest.mark.parametrize("t", [1, 127, 128, 129, 300])                         # around the 128-frame tile; three tiles
def test_raw_epilogue_conv_forward_and_data_gradient_match_float64(t, k):
    _lib, L = _api()
    x, w, dz, z_ref, dx_ref = _conv_reference(t, k)
    wk = _taps(w.float(), k).cuda()
    nbytes = L.ts_posconv_stack_conv_workspace(B, t, C, k)
    xs = x.float().cuda()
    z = _nan(B, t, C)
    ws = _ws(nbytes)
    assert L.ts_posconv_stack_conv(xs.data_ptr(), B, t, C, wk.to(BF).data_ptr(), k, G, 0, z.data_ptr(), ws.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    _assert_bf16_product(z, z_ref, f"stack conv forward t={t} k={k}")
    wb = wk.flip(0).transpose(2, 3).contiguous().to(BF)
    dzs = dz.float().cuda()
    dx = _nan(B, t, C)
    ws = _ws(nbytes)
    assert L.ts_posconv_stack_conv(dzs.data_ptr(), B, t, C, wb.data_ptr(), k, G, 1, dx.data_ptr(), ws.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    _assert_bf16_product(dx, dx_ref, f"stack conv data gradient t={t} k={k}")


def test_raw_epilogue_conv_refuses_what_the_kernel_cannot_do():
    _lib, L = _api()
    t, k = 16, 19
    x, out = torch.zeros(B * t * 192 + 8, device="cuda"), torch.zeros(B * t * 192, device="cuda")
    w = torch.zeros(k * 4 * 64 * 64, dtype=BF, device="cuda")
    ws = _ws(L.ts_posconv_stack_conv_workspace(B, t, 192, 512) + 16)
    call = lambda c, g, kk=k, xp=x.data_ptr(), wp=ws.data_ptr(): L.ts_posconv_stack_conv(xp, B, t, c, w.data_ptr(), kk, g, 0, out.data_ptr(), wp, _stream())
    assert call(192, 4) == _lib.TS_EUNSUPPORTED                               # 48 channels per group (data2vec-audio-base): the f32 GEMM branch of the node
    assert call(128, 2, kk=400) == _lib.TS_EUNSUPPORTED                       # (128 + 399) x 144 bytes > 64 KiB of LDS
    assert call(128, 2, xp=x.data_ptr() + 4) == _lib.TS_EUNSUPPORTED
    assert call(128, 2, wp=ws.data_ptr() + 4) == _lib.TS_EUNSUPPORTED
    assert call(128, 2, kk=1) == _lib.TS_EINVAL and call(128, 3) == _lib.TS_EINVAL and call(128, 0) == _lib.TS_EINVAL
    assert L.ts_posconv_stack_conv_workspace(B, 0, 128, k) == _lib.TS_EINVAL
    assert L.ts_posconv_stack_train_abi_version() == 1
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the kernel's two older epilogues
# ---------------------------------------------------------------------------------------------------------------------
def test_the_existing_matrix_core_entry_keeps_its_results_forward_and_backward():
    """ts_w2v_posconv_train at t = 129, k = 19 (the kernel is now a template with the raw epilogue as its other instantiation): y = x + gelu(conv + b) with the
    pre-activation z, and dx = dy + conv^T(dz), against the same float64 reference and bounds; two calls give equal bits."""
    _lib, L = _api()
    t, k = 129, 19
    x, w, dz, z_ref, dx_ref = _conv_reference(t, k)
    g = torch.Generator().manual_seed(3)
    bias, dy = 0.1 * torch.randn(C, generator=g), torch.randn(B, t, C, generator=g)
    wk = _taps(w.float(), k).cuda()
    wb = wk.flip(0).transpose(2, 3).contiguous().to(BF)
    xs, dzs, bs, dys = x.float().cuda(), dz.float().cuda(), bias.cuda(), dy.cuda()
    nbytes = L.ts_w2v_posconv_train_workspace(B, t, C, k)
    res = []
    for _ in range(2):
        y, z, dx = _nan(B, t, C), _nan(B, t, C), _nan(B, t, C)
        ws = _ws(nbytes)
        assert L.ts_w2v_posconv_train(xs.data_ptr(), xs.data_ptr(), B, t, C, wk.to(BF).data_ptr(), bs.data_ptr(), k, G, 0, y.data_ptr(), z.data_ptr(), ws.data_ptr(),
                                      _stream()) == 0
        ws2 = _ws(nbytes)
        assert L.ts_w2v_posconv_train(dzs.data_ptr(), dys.data_ptr(), B, t, C, wb.data_ptr(), None, k, G, 1, dx.data_ptr(), None, ws2.data_ptr(), _stream()) == 0
        torch.cuda.synchronize()
        res.append((y, z, dx))
    y, z, dx = res[0]
    _assert_bf16_product(z, z_ref, "posconv_train z")
    _assert_bf16_product(y, x.double() + F.gelu(z_ref + bias.double()), "posconv_train y")
    _assert_bf16_product(dx, dy.double() + dx_ref, "posconv_train dx")
    for a_, b_ in zip(res[0], res[1]):
        assert torch.equal(a_, b_)
    # and the raw epilogue leaves exactly the z of the older one: the same accumulator
    zr = _nan(B, t, C)
    ws = _ws(L.ts_posconv_stack_conv_workspace(B, t, C, k))
    assert L.ts_posconv_stack_conv(xs.data_ptr(), B, t, C, wk.to(BF).data_ptr(), k, G, 0, zr.data_ptr(), ws.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(zr, z)
