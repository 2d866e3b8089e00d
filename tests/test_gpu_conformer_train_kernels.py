"""The launches of wav2vec2-conformer fine-tuning (csrc/conformer_train.hip through include/thunder_speech_amd/conformer_train.h) on the raw C ABI against
float64 on the CPU: torch autograd in float64 through GLU -> depthwise conv -> BatchNorm -> activation for the convolution module, the written
formulas for the rotary transpose and the feed-forward activation pair.  Every output starts as NaN, every workspace as 0xFF bytes, every return
code is asserted, every launch runs twice and must give the same bits.

Bounds, the rule of tests/test_gpu_posconv_stack_kernels.py: f32 outputs within 1e-5 x max |reference|; activation values 1e-5 x max |reference| +
2e-6 BEFORE their rounding to bf16.  A bf16 output is compared with the reference rounded to bf16 and may be one bf16 ulp of that value away ON TOP of
the activation bound: got = bf16(a + e) with |e| <= E differs from bf16(a) by at most E plus half an ulp for each of the two roundings."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

NAN = float("nan")
EPS = 1e-5
ACTS = {1: F.gelu, 2: F.silu}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _api():
    from thunder_speech_amd import _lib
    return _lib, _lib.lib()


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def _ws(nbytes):
    assert nbytes > 0
    return torch.full((int(nbytes),), 0xFF, dtype=torch.uint8, device="cuda")


def _pad32(n):
    from thunder_speech_amd.huggingface.train import _pad32 as p
    return p(n)


def _assert_close(got, ref, rel, what, extra=0.0):
    got = got.detach().double().cpu()
    assert not bool(torch.isnan(got).any()), f"{what}: unwritten (NaN) elements"
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    err, scale = float((got - ref.double()).abs().max()), float(ref.abs().max())
    print(f"{what}: max error {err:.3e}, bound {rel * scale + extra:.3e}")
    assert err <= rel * scale + extra, f"{what}: max error {err:.3e} > {rel:.1e} x {scale:.3e} + {extra:.1e}"


def _assert_bf16(got, ref, what):
    """got (bf16) against the float64 activation `ref`: one bf16 ulp of bf16(ref) + the activation bound (module docstring)."""
    got = got.detach().float().double().cpu()
    assert not bool(torch.isnan(got).any()), f"{what}: unwritten (NaN) elements"
    r16 = ref.float().to(torch.bfloat16).double()
    ulp = torch.exp2(torch.floor(torch.log2(r16.abs().clamp_min(2.0 ** -126))) - 7.0)
    bound = ulp + 1e-5 * float(ref.abs().max()) + 2e-6
    over = (got - r16).abs() - bound
    print(f"{what}: worst excess over one bf16 ulp + activation bound {float(over.max()):.3e}; elements off by more than the activation bound: "
          f"{int(((got - r16).abs() > 1e-5 * float(ref.abs().max()) + 2e-6).sum())} of {got.numel()}")
    assert float(over.max()) <= 0.0, f"{what}: {float(over.max()):.3e} over the bound"


def _conv_reference(u, dw, gamma, beta, da, act, running=None, eps=EPS):
    """float64 autograd through the convolution module's core.  -> dict of z, mean, var, rstd, a, du, ddw, dgamma, dbeta."""
    b, t, c2 = u.shape
    c, k = c2 // 2, dw.shape[0]
    ur, wr = u.double().requires_grad_(True), dw.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    glu = ur[..., :c] * torch.sigmoid(ur[..., c:])
    z = F.conv1d(glu.transpose(1, 2), wr.t().unsqueeze(1), padding=(k - 1) // 2, groups=c).transpose(1, 2)
    if running is None:
        mean, var = z.mean((0, 1)), z.var((0, 1), unbiased=False)
        rstd = 1.0 / torch.sqrt(var + eps)
    else:
        mean, rstd = running[0].double(), running[1].double()
        var = None
    a = ACTS[act](gr * (z - mean) * rstd + br)
    (a * da.double()).sum().backward()
    return dict(z=z.detach(), mean=mean.detach(), var=None if var is None else var.detach(), rstd=rstd.detach(), a=a.detach(), du=ur.grad, ddw=wr.grad,
                dgamma=gr.grad, dbeta=br.grad)


def _conv_inputs(b, t, c, k, seed):
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(b, t, 2 * c, generator=g)
    dw = torch.randn(k, c, generator=g) / math.sqrt(k)
    gamma = 1.0 + 0.1 * torch.randn(c, generator=g)
    beta = 0.1 * torch.randn(c, generator=g)
    da = torch.randn(b, t, c, generator=g)
    return u, dw, gamma, beta, da


def _conv_forward(u, dw, gamma, beta, act, running=None, eps=EPS):
    """The three forward launches, twice.  -> (z, mean_rstd, mean_var or None, y16, yt16) on the GPU."""
    _lib, L = _api()
    b, t, c2 = u.shape
    c, k = c2 // 2, dw.shape[0]
    rows, rp = b * t, _pad32(b * t)
    u_, dw_, g_, b_ = u.cuda(), dw.cuda(), gamma.cuda(), beta.cuda()
    runs = []
    for _ in range(2):
        z, ws = _nan(b, t, c), _ws(L.ts_conformer_glu_dwconv_train_fwd_workspace(b, t, c))
        assert L.ts_conformer_glu_dwconv_train_fwd(u_.data_ptr(), b, t, c, dw_.data_ptr(), k, z.data_ptr(), ws.data_ptr(), _stream()) == 0
        if running is None:
            mean_rstd, mean_var = _nan(2, c), _nan(2, c)
            assert L.ts_conformer_bn_stats(ws.data_ptr(), b, t, c, eps, mean_rstd.data_ptr(), mean_var.data_ptr(), _stream()) == 0
        else:
            mean_rstd, mean_var = running.cuda().contiguous(), None
        y16, yt16 = _nan(rows, c, dtype=torch.bfloat16), _nan(c, rp, dtype=torch.bfloat16)
        assert L.ts_conformer_bn_act_cast(z.data_ptr(), mean_rstd.data_ptr(), g_.data_ptr(), b_.data_ptr(), rows, c, act, y16.data_ptr(), yt16.data_ptr(),
                                          rp, rp, _stream()) == 0
        torch.cuda.synchronize()
        runs.append((z, mean_rstd, mean_var, y16, yt16))
    for x0, x1 in zip(*runs):
        assert x0 is None or torch.equal(x0, x1), "two forward runs differ"
    return runs[0]


def _conv_backward(u, dw, gamma, beta, da, act, z, mean_rstd, running):
    """The two backward entry points on the GPU's own z and statistics, twice.  -> (dgamma, dbeta, du, ddw)."""
    _lib, L = _api()
    b, t, c2 = u.shape
    c, k = c2 // 2, dw.shape[0]
    rows = b * t
    u_, dw_, g_, b_, da_ = u.cuda(), dw.cuda(), gamma.cuda(), beta.cuda(), da.cuda()
    runs = []
    for _ in range(2):
        dgamma, dbeta = _nan(c), _nan(c)
        ws = _ws(L.ts_conformer_bn_act_bwd_sums_workspace(rows, c))
        assert L.ts_conformer_bn_act_bwd_sums(z.data_ptr(), mean_rstd.data_ptr(), g_.data_ptr(), b_.data_ptr(), da_.data_ptr(), rows, c, act,
                                              dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(), _stream()) == 0
        du, ddw = _nan(b, t, 2 * c), _nan(k, c)
        ws = _ws(L.ts_conformer_glu_dwconv_train_bwd_workspace(b, t, c, k))
        assert L.ts_conformer_glu_dwconv_train_bwd(u_.data_ptr(), z.data_ptr(), da_.data_ptr(), b, t, c, dw_.data_ptr(), k, mean_rstd.data_ptr(),
                                                   g_.data_ptr(), b_.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), int(running), act, du.data_ptr(),
                                                   ddw.data_ptr(), ws.data_ptr(), _stream()) == 0
        torch.cuda.synchronize()
        runs.append((dgamma, dbeta, du, ddw))
    for x0, x1 in zip(*runs):
        assert torch.equal(x0, x1), "two backward runs differ"
    return runs[0]


# (1, 8, 64, 31): a clip shorter than the halo; (2, 130, 64, 5): two frames past a 128-frame tile; (1, 257, 192, 63): the tap-loop kernel, three tiles
SHAPES = [(1, 8, 64, 31), (2, 130, 64, 5), (3, 199, 128, 31), (1, 257, 192, 63), (2, 129, 64, 3)]


@pytest.mark.parametrize("act", [1, 2])
@pytest.mark.parametrize("b,t,c,k", SHAPES)
def test_conv_module_forward_and_backward_with_batch_statistics(b, t, c, k, act):
    u, dw, gamma, beta, da = _conv_inputs(b, t, c, k, seed=1000 * t + 10 * k + act)
    ref = _conv_reference(u, dw, gamma, beta, da, act)
    z, mean_rstd, mean_var, y16, yt16 = _conv_forward(u, dw, gamma, beta, act)
    what = f"B={b} t={t} c={c} k={k} act={act}"
    _assert_close(z, ref["z"], 1e-5, what + " z")
    _assert_close(mean_rstd[0], ref["mean"], 1e-5, what + " mean")
    _assert_close(mean_var[0], ref["mean"], 1e-5, what + " mean (second copy)")
    _assert_close(mean_rstd[1], ref["rstd"], 1e-5, what + " rstd")
    _assert_close(mean_var[1], ref["var"], 1e-5, what + " biased variance")
    rows = b * t
    _assert_bf16(y16.view(b, t, c), ref["a"], what + " operand")
    _assert_bf16(yt16[:, :rows].t().reshape(b, t, c), ref["a"], what + " transposed operand")
    assert float(yt16[:, rows:].float().abs().max()) == 0.0 if yt16.shape[1] > rows else True, what + ": padding rows of the transposed operand"
    assert torch.equal(yt16[:, :rows].t().contiguous(), y16), what + ": the two operand copies differ"
    dgamma, dbeta, du, ddw = _conv_backward(u, dw, gamma, beta, da, act, z, mean_rstd, running=False)
    _assert_close(dgamma, ref["dgamma"], 1e-5, what + " dgamma")
    _assert_close(dbeta, ref["dbeta"], 1e-5, what + " dbeta")
    _assert_close(du, ref["du"], 1e-5, what + " du")
    _assert_close(ddw, ref["ddw"], 1e-5, what + " d dw_w")


@pytest.mark.parametrize("act", [1, 2])
@pytest.mark.parametrize("b,t,c,k", SHAPES)
def test_conv_module_forward_and_backward_with_running_statistics(b, t, c, k, act):
    u, dw, gamma, beta, da = _conv_inputs(b, t, c, k, seed=2000 * t + 10 * k + act)
    g = torch.Generator().manual_seed(t)
    running = torch.stack([0.1 * torch.randn(c, generator=g), 1.0 / torch.sqrt(torch.rand(c, generator=g) + 0.5 + EPS)])
    ref = _conv_reference(u, dw, gamma, beta, da, act, running=running)
    z, mean_rstd, _, y16, yt16 = _conv_forward(u, dw, gamma, beta, act, running=running)
    what = f"running B={b} t={t} c={c} k={k} act={act}"
    _assert_close(z, ref["z"], 1e-5, what + " z")
    _assert_bf16(y16.view(b, t, c), ref["a"], what + " operand")
    assert torch.equal(yt16[:, :b * t].t().contiguous(), y16)
    dgamma, dbeta, du, ddw = _conv_backward(u, dw, gamma, beta, da, act, z, mean_rstd, running=True)
    _assert_close(dgamma, ref["dgamma"], 1e-5, what + " dgamma")
    _assert_close(dbeta, ref["dbeta"], 1e-5, what + " dbeta")
    _assert_close(du, ref["du"], 1e-5, what + " du")
    _assert_close(ddw, ref["ddw"], 1e-5, what + " d dw_w")


def test_batch_statistics_of_channels_whose_mean_is_fifty_standard_deviations():
    """z = u1 sigmoid(30) = u1 exactly in f32 (k = 1, tap 1), channel means of 50 standard deviations, n = 2 x 199 = 398: rstd within 1e-5 relative of
    float64.  On the CPU first: float32 E[x^2] - E[x]^2 of the same values misses that bound (2 500 x 2^-24 relative in the variance) and float32 Chan
    over 128-frame blocks holds it, so the bound tells the two apart."""
    _lib, L = _api()
    b, t, c = 2, 199, 64
    g = torch.Generator().manual_seed(7)
    sig = torch.rand(c, generator=g) + 0.5
    x = (50.0 * sig + sig * torch.randn(b, t, c, generator=g)).float()
    ref_var = x.double().var((0, 1), unbiased=False)
    ref_rstd = 1.0 / torch.sqrt(ref_var + EPS)
    flat = x.view(-1, c)
    naive = 1.0 / torch.sqrt(((flat * flat).mean(0) - flat.mean(0) ** 2) + EPS)
    assert float(((naive.double() - ref_rstd) / ref_rstd).abs().max()) > 1e-5
    n, mean, m2 = 0, torch.zeros(c), torch.zeros(c)
    for blk in flat.split(128):
        nb, mb = blk.shape[0], blk.mean(0)
        d, tot = mb - mean, n + blk.shape[0]
        mean, m2, n = mean + d * (nb / tot), m2 + ((blk - mb) ** 2).sum(0) + d * d * (n * nb / tot), tot
    chan = 1.0 / torch.sqrt(m2 / n + EPS)
    assert float(((chan.double() - ref_rstd) / ref_rstd).abs().max()) < 1e-5
    u = torch.cat([x, torch.full((b, t, c), 30.0)], -1)
    assert torch.equal((u[..., :c] * torch.sigmoid(u[..., c:])), x)
    z, mean_rstd, mean_var, _, _ = _conv_forward(u, torch.ones(1, c), torch.ones(c), torch.zeros(c), 2)
    assert torch.equal(z.cpu(), x)
    rel = ((mean_rstd[1].double().cpu() - ref_rstd) / ref_rstd).abs().max()
    print("shifted mean: rstd relative error", float(rel), "variance", float(((mean_var[1].double().cpu() - ref_var) / ref_var).abs().max()))
    assert float(rel) <= 1e-5
    assert float(((mean_var[1].double().cpu() - ref_var) / ref_var).abs().max()) <= 1e-5
    _assert_close(mean_rstd[0], x.double().mean((0, 1)), 1e-5, "shifted mean: mean")


@pytest.mark.parametrize("act", [1, 2])
def test_two_frames_are_enough_for_batch_statistics(act):
    """B = 1, t = 2, eps = 0.1.  With two values per channel zh^2 = var / (var + eps), and BatchNorm's data gradient
    g - mean(g) - zh mean(g zh) = (g1 - g2) / 2 x eps / (var + eps) is what is left of a cancellation: float32 resolves it to about 2^-24 |g| whatever
    the kernel does.  With the module default eps = 1e-5 that is the WHOLE gradient of a channel whose two values differ by more than a few hundredths
    (random inputs, measured: d dw_w 1.2e-5 off at a largest reference of 0.76; float32 torch autograd on the CPU is 1.0e-5 off on the same inputs), so there
    the 1e-5 bound would test float32, not the kernel.  eps is an argument; at 0.1 every channel's gradient is a tenth or more of g and the bound speaks about the launches."""
    b, t, c, k, eps = 1, 2, 64, 3, 0.1
    u, dw, gamma, beta, da = _conv_inputs(b, t, c, k, seed=5 + act)
    ref = _conv_reference(u, dw, gamma, beta, da, act, eps=eps)
    z, mean_rstd, mean_var, y16, _ = _conv_forward(u, dw, gamma, beta, act, eps=eps)
    _assert_close(z, ref["z"], 1e-5, "n=2 z")
    _assert_close(mean_rstd[1], ref["rstd"], 1e-5, "n=2 rstd")
    _assert_close(mean_var[1], ref["var"], 1e-5, "n=2 variance")
    _assert_bf16(y16.view(b, t, c), ref["a"], "n=2 operand")
    dgamma, dbeta, du, ddw = _conv_backward(u, dw, gamma, beta, da, act, z, mean_rstd, running=False)
    for got, name in ((dgamma, "dgamma"), (dbeta, "dbeta"), (du, "du"), (ddw, "ddw")):
        _assert_close(got, ref[name], 1e-5, "n=2 " + name)


# ---- rotary transpose ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,t,c", [(2, 7, 128), (1, 300, 192)])
def test_rotary_transpose_matches_float64_and_is_the_adjoint_of_the_forward_launch(b, t, c):
    from thunder_speech_amd.huggingface.conformer import rotary_table
    _lib, L = _api()
    t_table = t + 13
    g = torch.Generator().manual_seed(b * t + c)
    inv_freq = 1.0 / (10000 ** (torch.arange(0, 64, 2).float() / 64))
    table = rotary_table(inv_freq, t_table)                                    # [2][t_table][32]
    dv, dr = torch.randn(b, t, c, generator=g), torch.randn(b, t, c, generator=g)
    cos = table[0, :t].double().repeat(1, c // 32)[None]                       # [1][t][c]: column j -> frequency j % 32
    sin = table[1, :t].double().repeat(1, c // 32)[None]
    j = torch.arange(c)
    partner, s = j ^ 32, torch.where(j % 64 < 32, -1.0, 1.0).double()
    ref = dv.double() + dr.double() * cos - s * dr.double()[..., partner] * sin
    tb, dv_, dr_ = table.cuda(), dv.cuda(), dr.cuda()
    outs = []
    for _ in range(2):
        dy = _nan(b, t, c)
        assert L.ts_conformer_rotary_bwd(dv_.data_ptr(), dr_.data_ptr(), b, t, c, tb.data_ptr(), t_table, dy.data_ptr(), _stream()) == 0
        torch.cuda.synchronize()
        outs.append(dy)
    assert torch.equal(outs[0], outs[1])
    _assert_close(outs[0], ref, 1e-5, f"rotary transpose B={b} t={t} c={c}")
    # <rot(y), w> = <y, rot^T(w)> with y, rot(y) the two outputs of ONE forward launch and rot^T(w) = the transpose launch with a zero value branch.
    # Both sides are summed in float64 from the f32 results, so only the elements' own rounding counts: an element of either launch is a sum of two
    # products, at most three roundings: |error| <= gamma_3 (|y_j| + |y_partner|) (|cos|, |sin| <= 1), gamma_3 = 3 u / (1 - 3 u), u = 2^-24.  Over
    # the dot product and for both sides: tol = 2 gamma_3 sum_j |w_j| (|y_j| + |y_partner(j)|).
    x = torch.randn(b, t, c, generator=g).cuda()
    w = torch.randn(b, t, c, generator=g).cuda()
    lw, lb = (1.0 + 0.1 * torch.randn(c, generator=g)).cuda(), (0.1 * torch.randn(c, generator=g)).cuda()
    y, yr, wt = _nan(b, t, c), _nan(b, t, c), _nan(b, t, c)
    assert L.ts_conformer_layernorm_rotary_fwd(x.data_ptr(), lw.data_ptr(), lb.data_ptr(), 1e-5, b, t, c, c // 64, tb.data_ptr(), t_table, 0, y.data_ptr(),
                                               yr.data_ptr(), _stream()) == 0
    zero = torch.zeros(b, t, c, device="cuda")
    assert L.ts_conformer_rotary_bwd(zero.data_ptr(), w.data_ptr(), b, t, c, tb.data_ptr(), t_table, wt.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    y, yr, w, wt = (v.double().cpu() for v in (y, yr, w, wt))
    lhs, rhs = float((yr * w).sum()), float((y * wt).sum())
    u_ = 2.0 ** -24
    tol = 2.0 * (3 * u_ / (1 - 3 * u_)) * float((w.abs() * (y.abs() + y[..., partner].abs())).sum())
    print(f"adjoint identity: {lhs} against {rhs}, |difference| {abs(lhs - rhs):.3e}, tolerance {tol:.3e}")
    assert abs(lhs - rhs) <= tol


# ---- the act-aware feed-forward pair ------------------------------------------------------------------------------------------------------------
def _ffn_pair(L, cast, bwd, z, bias, da, p, seed, act=None):
    rows, c = z.shape
    rp = _pad32(rows)
    outs = []
    for _ in range(2):
        y16, yt16, dz = _nan(rows, c, dtype=torch.bfloat16), _nan(c, rp, dtype=torch.bfloat16), _nan(rows, c)
        extra = () if act is None else (act,)
        assert cast(z.data_ptr(), bias.data_ptr(), rows, c, *extra, p, seed, y16.data_ptr(), yt16.data_ptr(), rp, rp, _stream()) == 0
        assert bwd(z.data_ptr(), bias.data_ptr(), c, *extra, da.data_ptr(), p, seed, dz.data_ptr(), rows * c, _stream()) == 0
        torch.cuda.synchronize()
        outs.append((y16, yt16, dz))
    for x0, x1 in zip(*outs):
        assert torch.equal(x0.view(torch.int16) if x0.dtype == torch.bfloat16 else x0, x1.view(torch.int16) if x1.dtype == torch.bfloat16 else x1)
    return outs[0]


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("rows,c", [(70, 256), (199, 132)])
def test_ffn_activation_pair_with_the_gelu_code_gives_the_bits_of_the_wav2vec2_pair(rows, c, p):
    _lib, L = _api()
    g = torch.Generator().manual_seed(rows + c)
    z, bias, da = torch.randn(rows, c, generator=g).cuda(), torch.randn(c, generator=g).cuda(), torch.randn(rows, c, generator=g).cuda()
    old = _ffn_pair(L, L.ts_w2v_ffn_act_cast, L.ts_w2v_ffn_act_bwd, z, bias, da, p, 1234)
    new = _ffn_pair(L, L.ts_conformer_ffn_act_cast, L.ts_conformer_ffn_act_bwd, z, bias, da, p, 1234, act=1)
    for a, b_ in zip(old, new):
        assert not bool(torch.isnan(a.float()).any())
        assert torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a, b_.view(torch.int16) if b_.dtype == torch.bfloat16 else b_)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("rows,c", [(70, 256), (199, 132)])
def test_ffn_activation_pair_with_the_silu_code_matches_float64_under_the_philox_mask(rows, c, p):
    from oracle import philox as ph
    _lib, L = _api()
    g = torch.Generator().manual_seed(3 * rows + c)
    z, bias, da = 2.0 * torch.randn(rows, c, generator=g), torch.randn(c, generator=g), torch.randn(rows, c, generator=g)
    seed = 99
    keep = torch.ones(rows, c, dtype=torch.float64)
    if p > 0:
        keep = torch.from_numpy(np.asarray(ph.dropout_keep(seed, rows * c, p)).astype(np.float64)[:rows * c]).view(rows, c) / (1.0 - np.float32(p).astype(np.float64))
        assert 0.05 < 1.0 - float((keep > 0).double().mean()) < 0.15
    zr = (z.double() + bias.double()).requires_grad_(True)
    a = F.silu(zr) * keep
    (a * da.double()).sum().backward()
    y16, yt16, dz = _ffn_pair(L, L.ts_conformer_ffn_act_cast, L.ts_conformer_ffn_act_bwd, z.cuda(), bias.cuda(), da.cuda(), p, seed, act=2)
    _assert_bf16(y16, a.detach(), f"silu pair rows={rows} c={c} p={p} operand")
    assert torch.equal(yt16[:, :rows].t().contiguous().view(torch.int16), y16.view(torch.int16))
    if yt16.shape[1] > rows:
        assert float(yt16[:, rows:].float().abs().max()) == 0.0
    _assert_close(dz, zr.grad, 1e-5, f"silu pair rows={rows} c={c} p={p} dz")


# ---- argument checks ---------------------------------------------------------------------------------------------------------------------------
def test_argument_checks_return_before_any_launch():
    """TS_EINVAL: NULL pointers; B, t, c <= 0; n < 2 for batch statistics; t > t_table.  TS_EUNSUPPORTED: an even kernel or one above 63; c % 64 != 0 for
    the rotary launch and c % 8 != 0 elsewhere; act not 1 or 2; misaligned pointers; B > 65535.  Real (small) buffers: a call that wrongly launched would
    still stay inside them."""
    _lib, L = _api()
    E, U = _lib.TS_EINVAL, _lib.TS_EUNSUPPORTED
    buf = torch.zeros(1 << 16, device="cuda")
    A, M, s = buf.data_ptr(), buf.data_ptr() + 4, _stream()
    fwd = lambda u=A, b=1, t=8, c=64, w=A, k=3, z=A, ws=A: L.ts_conformer_glu_dwconv_train_fwd(u, b, t, c, w, k, z, ws, s)
    stats = lambda ws=A, b=1, t=8, c=64, mr=A, mv=A: L.ts_conformer_bn_stats(ws, b, t, c, EPS, mr, mv, s)
    cast = lambda z=A, mr=A, g=A, be=A, rows=8, c=64, act=2, y=A, yt=A, ldt=32, rp=32: L.ts_conformer_bn_act_cast(z, mr, g, be, rows, c, act, y, yt, ldt, rp, s)
    sums = lambda z=A, mr=A, g=A, be=A, da=A, rows=8, c=64, act=2, dg=A, db=A, ws=A: L.ts_conformer_bn_act_bwd_sums(z, mr, g, be, da, rows, c, act, dg, db, ws, s)
    bwd = lambda u=A, z=A, da=A, b=1, t=8, c=64, w=A, k=3, mr=A, g=A, be=A, dg=A, db=A, run=0, act=2, du=A, ddw=A, ws=A: \
        L.ts_conformer_glu_dwconv_train_bwd(u, z, da, b, t, c, w, k, mr, g, be, dg, db, run, act, du, ddw, ws, s)
    rot = lambda dv=A, dr=A, b=1, t=8, c=64, cs=A, tt=8, dy=A: L.ts_conformer_rotary_bwd(dv, dr, b, t, c, cs, tt, dy, s)
    for name in ("u", "w", "z", "ws"):
        assert fwd(**{name: 0}) == E, name
    for name in ("ws", "mr", "mv"):
        assert stats(**{name: 0}) == E, name
    for name in ("z", "mr", "g", "be"):
        assert cast(**{name: 0}) == E, name
    assert cast(y=0, yt=0) == E
    for name in ("z", "mr", "g", "be", "da", "dg", "db", "ws"):
        assert sums(**{name: 0}) == E, name
    for name in ("u", "z", "da", "w", "mr", "g", "be", "dg", "db", "du", "ddw", "ws"):
        assert bwd(**{name: 0}) == E, name
    for name in ("dv", "dr", "cs", "dy"):
        assert rot(**{name: 0}) == E, name
    for f in (fwd, stats, bwd, rot):
        for kw in (dict(b=0), dict(b=-1), dict(t=0), dict(c=0), dict(c=-64)):
            assert f(**kw) == E, (f, kw)
    for f in (cast, sums):
        assert f(rows=0) == E and f(c=0) == E
    assert stats(b=1, t=1) == E and bwd(b=1, t=1) == E and bwd(b=1, t=1, run=1) == 0      # n < 2: batch statistics only
    assert rot(t=9, tt=8) == E
    assert L.ts_conformer_glu_dwconv_train_fwd_workspace(0, 8, 64) == E and L.ts_conformer_bn_act_bwd_sums_workspace(0, 64) == E
    assert L.ts_conformer_glu_dwconv_train_bwd_workspace(1, 8, 0, 3) == E
    for k in (2, 4, 30, 65, 0, -1):
        assert fwd(k=k) == U and bwd(k=k) == U and L.ts_conformer_glu_dwconv_train_bwd_workspace(1, 8, 64, k) == U, k
    for f in (fwd, stats, cast, sums, bwd):
        assert f(c=68) == U, f
    assert rot(c=72) == U and rot(c=32) == U
    for act in (0, 3, -1):
        assert cast(act=act) == U and sums(act=act) == U and bwd(act=act) == U
    for f, names in ((fwd, ("u", "w", "z", "ws")), (stats, ("ws", "mr", "mv")), (cast, ("z", "mr", "g", "be", "y", "yt")),
                     (sums, ("z", "mr", "g", "be", "da", "dg", "db", "ws")),
                     (bwd, ("u", "z", "da", "w", "mr", "g", "be", "dg", "db", "du", "ddw", "ws")), (rot, ("dv", "dr", "cs", "dy"))):
        for name in names:
            assert f(**{name: M}) == U, (f, name)
    for f in (fwd, stats, bwd, rot):
        assert f(b=65536) == U, f
    for act in (0, 3):
        assert L.ts_conformer_ffn_act_cast(A, A, 8, 64, act, 0.0, 1, A, A, 32, 32, s) == U
        assert L.ts_conformer_ffn_act_bwd(A, A, 64, act, A, 0.0, 1, A, 512, s) == U
    assert L.ts_conformer_ffn_act_cast(0, A, 8, 64, 2, 0.0, 1, A, A, 32, 32, s) == E and L.ts_conformer_ffn_act_bwd(A, A, 64, 2, 0, 0.0, 1, A, 512, s) == E
    torch.cuda.synchronize()
