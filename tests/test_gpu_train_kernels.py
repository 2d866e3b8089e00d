"""Every QuartzNet / Citrinet training kernel of csrc/train_dw.hip, train_bn.hip, train_rows.hip, train_extra.hip (rows of csrc/train_act.hpp) through
the C ABI against a plain float64 restatement on the CPU (F.conv1d, means, autograd; nothing of thunder_speech_amd), at the shapes where the dispatch
changes: one and several 512-frame row units per row with idle waves in the last workgroup, empty / single / uneven BatchNorm clip groups, the pair,
matrix-core and tile-statistics forms of the depthwise forward with the BatchNorm input, two row pairs per wave, one and several clips per wave of the
pair backward, the general-geometry kernels across their 1024-frame tile, the phase-split (dilation 2) kernels on a pitch that is no multiple of 16,
the deterministic mode, the three precisions of the pointwise products.

Conventions of every case: every return code is asserted; every output buffer starts as NaN with one guard row (7.0) behind it that must come back
bit for bit; the inputs carry NaN in their columns >= t (the header calls them scratch); inputs that are bf16 on the device are rounded first and
the restatement reads the rounded values; both `act` values run.

Bounds (one per kind of output; `max` = max |reference| over the tensor):
  f32 rows, forward (BatchNorm apply, add, SE scale, depthwise)       2e-5 x max                       (what the block-tail test holds on this hardware)
  f32 gradients, f32 parameter gradients formed from exact inputs     1e-4 x max                       (same source)
  dv of the BatchNorm backward                                        the gradient bound + 8 x 2^-24 x gamma rstd (|g| + |mean g| + (|xhat| + |mean| rstd)
                                                                      |mean(g xhat)|): dv = gamma rstd (g - mean g - xhat mean(g xhat)) cancels -- with
                                                                      n = 2 frames down to eps / var of g -- and every f32 term is rounded at its own size
  clip-group sums of ts_train_bn_stats (doubles)                      1e-6 x sum |v| and 1e-6 x sum v^2 of the group: 8 terms are added in f32, then
                                                                      f64 accumulates, so the error is <= 8 x 2^-24 of the absolute sum
  published mean_rstd                                                 mean: 1e-6 x mean |v| + 2^-23 |mean|;  rstd: 1e-5 relative for inputs with
                                                                      spread 2 around mean 3 (E[v^2] / var = 3.25: the cancellation in s2 / n - m^2
                                                                      stays below 4e-6); in general 1e-6 x E[v^2] / var (the mean-of-fifty-spreads
                                                                      case: E[v^2] / var = 2501)
  running statistics                                                  rtol 1e-5 against 0.9 old + 0.1 new with the unbiased variance n / (n - 1);
                                                                      the counter moves by exactly 1; they start from random values
  bf16 rows                                                           per element |got - ref| <= 2^-8 |ref| + (the f32 bound of that output)
  ts_train_cast_bf16, ts_train_act_import(act = 1)                    bit-equal to torch's round-to-nearest-even (finite values, ties, -0.0, extremes)
  ts_train_act_export, act_import(act = 0), masks, relu_bwd, subsample_mask      bit-equal
  in_dgamma / in_dbeta of ts_train_dwconv_bwd_bn at act 1             4e-3 x max                       (the figure of test_gpu_dw_bwd_mfma.py)
  row sums (ts_train_se_pool, ts_train_se_rowdot), f32                (ceil(t / 64) + 9) x 2^-24 x sum |terms| of the row (/ t for the mean): a lane adds
                                                                      ceil(t / 64) terms, six shuffle steps combine the lanes, one product / division
  pointwise products                                                  precision 0: the f32 bounds above; bf16 operands: 2e-3 x max for f32 results,
                                                                      6e-3 x max for bf16 results (test_bf16_pointwise_products_match_a_float64_product)
  matrix-core depthwise forward                                       the reference rounds the taps to bf16, as that kernel does.  With the BatchNorm
                                                                      input the kernel also rounds the normalised frames x to bf16 -- they are the
                                                                      MFMA's B operand, and bf16 is what the two-step path would have stored -- so each
                                                                      product carries up to 2^-8 |w x| (the unit roundoff of bf16) and the bound gains
                                                                      2^-8 (1 + 2^-8) x (|w| * |x|)[t] per element: the convolution of the absolute
                                                                      values, and the stored bf16 then rounds the perturbed value.  A derived term,
                                                                      not a measured one
  matrix-core depthwise backward (deterministic-mode case only)       dx 6e-3 x max, dw 1e-5 x max, sums 4e-3 x max: test_gpu_dw_bwd_mfma.py's own; dw gains
                                                                      2^-8 x sum |dy| |x| per tap, the bf16 staging of the normalised x as in the forward

ReLU gates that a kernel recomputes (ts_train_dwconv_bwd_bn forms relu'(v sc + hs) itself): v is built so that no float64 pre-activation lies within
1e-4 of zero (offending elements are drawn again, after rounding for bf16), asserted before the launch; no element is left out of a comparison.
Where the gate is an input (y of ts_train_bn_bwd, out of ts_train_relu_bwd) the reference's own rounded output is handed in.

Every check prints `RATIO|kind|error / bound` before it asserts (profiles/train_kernel_checks.md is collected from these lines); the float64 restatements
dominate the running time."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

NAN = float("nan")
BF = torch.bfloat16
DT = {0: torch.float32, 1: BF}
GUARD = 7.0
EPS = 1e-3
U24 = 2.0 ** -24


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _api():
    from thunder_speech_amd import _lib
    return _lib, _lib.lib()


def _ptr(x):
    return None if x is None else x.data_ptr()


_KEPT = []


def _keep(x):
    """address of a device tensor that lives to the end of the test: a temporary is freed as soon as data_ptr() has returned, BEFORE the launch,
    and the next temporary of the same argument list may be handed the same block (gamma and beta then share one address)"""
    _KEPT.append(x)
    return x.data_ptr()


def _dev(x):
    return _keep(x.cuda())


@pytest.fixture(autouse=True)
def _release_kept():
    yield
    _KEPT.clear()


def _r8(n):
    return (n + 7) // 8 * 8


def _rnd(x, act):
    """what the device holds of x: rounded to bf16 for act 1"""
    return x.float().to(DT[act]).float()


def _in_rows(x, pitch, act):
    """x f32 [..., t] (already rounded) -> device rows [..., pitch] of the call's element type, NaN from column t on"""
    t = x.shape[-1]
    buf = torch.full((*x.shape[:-1], pitch), NAN, dtype=DT[act], device="cuda")
    buf[..., :t] = x.to(DT[act]).cuda()
    return buf


def _out(rows, width, dtype=torch.float32):
    """[rows + 1][width]: NaN everywhere, the last row is the guard"""
    buf = torch.full((rows + 1, width), NAN, dtype=dtype, device="cuda")
    buf[rows] = GUARD
    return buf


def _start(x):
    """an accumulating f32 output: the rows of x (CPU) and a guard row behind them"""
    x = x.float().reshape(x.shape[0], -1)
    buf = _out(x.shape[0], x.shape[1])
    buf[:-1] = x.cuda()
    return buf


def _guard_ok(buf, what):
    assert bool((buf[-1] == GUARD).all()), f"{what}: the guard row behind the output was written"


def _bits(x):
    x = x.contiguous()
    return x.view(torch.int16 if x.dtype == BF else torch.int32)


def _assert_bits(got, want, what):
    """bit-equal (a NaN, an unwritten element, differs from every finite pattern)"""
    got = got.detach().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.equal(_bits(got), _bits(want.to(got.dtype))), f"{what}: not bit-equal"


def _check(got, ref, rel, kind, what, bf16=False, extra=None):
    """per element |got - ref| <= rel x max |ref| (+ 2^-8 |ref| for bf16 rows) (+ extra); a NaN anywhere (an unwritten element) fails"""
    got, ref = got.detach().double().cpu(), ref.detach().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert not bool(torch.isnan(got).any()), f"{what}: unwritten (NaN) elements"
    bound = torch.full_like(ref, rel * float(ref.abs().max()) if ref.numel() else 0.0)
    if bf16:
        bound = bound + 2.0 ** -8 * ref.abs()
    if extra is not None:
        bound = bound + extra
    _report(kind, what, (got - ref).abs(), bound)


def _report(kind, what, err, bound):
    if err.numel() == 0:
        return
    ratio = float((err / bound.clamp_min(1e-300)).max()) if bool((bound > 0).any()) else 0.0
    worst = int((err - bound).argmax())
    print(f"RATIO|{kind}|{ratio:.3e}|{what}")
    assert bool((err <= bound).all()), (f"{what}: error {float(err.flatten()[worst]):.3e} > bound {float(bound.flatten()[worst]):.3e} at flat index {worst} "
                                        f"(largest error / bound {ratio:.3e})")


def _mask(lens, t):
    """[B][1][t] float64: frames < clamp(len, 0, t)"""
    return (torch.arange(t)[None, :] < lens.long().clamp(0, t)[:, None]).double()[:, None, :]


# ---------------------------------------------------------------------------------------------------------------------
# 1. row kernels: one wave per (row, 512-frame chunk), four units per workgroup, 8 frames per lane
# ---------------------------------------------------------------------------------------------------------------------
ROW_T = [1, 7, 8, 9, 511, 512, 513, 1025]
ROW_BC = [(1, 1), (1, 3), (5, 1)]                                             # 1, 3 and 5 rows: the last workgroup has idle waves


def _pitches(t):
    return (_r8(t), _r8(t) + 64)


def _len_sets(batch, t):
    vals = [0, 1, t - 1, t, t + 5, -3]                                       # the kernels clamp to [0, t]
    return [[v] for v in vals] if batch == 1 else [vals[:5], [-3, t, 1, t + 5, 0]]


def _row_shapes(t):
    return [(b, c, p) for b, c in ROW_BC for p in _pitches(t)]


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("t", ROW_T)
def test_mask_time_is_bit_equal(t, act):
    """ts_train_mask_time: y = x for frames < clamp(len), +0.0 behind; pitch_x != pitch_y"""
    _lib, L = _api()
    for b, c, p in _row_shapes(t):
        g = torch.Generator().manual_seed(t + 10 * b + c)
        x = _rnd(torch.randn(b, c, t, generator=g), act)
        x[..., 0] = -0.0
        xd = _in_rows(x, p, act)
        for lens in _len_sets(b, t):
            ln = torch.tensor(lens, dtype=torch.int32)
            y = _out(b * c, p + 8, DT[act])
            assert L.ts_train_mask_time(xd.data_ptr(), _dev(ln), y.data_ptr(), b, c, t, p, p + 8, act, _stream()) == 0
            torch.cuda.synchronize()
            what = f"mask_time b={b} c={c} t={t} pitch={p} len={lens} act={act}"
            want = torch.where(_mask(ln, t).bool().expand(b, c, t), x, torch.zeros_like(x))
            _assert_bits(y[:-1, :t].view(b, c, t), want, what)
            _guard_ok(y, what)
    assert L.ts_train_mask_time(xd.data_ptr(), None, y.data_ptr(), b, c, t, p, p + 8, act, _stream()) == _lib.TS_EINVAL


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("t", ROW_T)
def test_add_with_and_without_the_length_of_b(t, act):
    """ts_train_add: out = a + mask(b, len_b[row / channels])"""
    _lib, L = _api()
    for b, c, p in _row_shapes(t):
        g = torch.Generator().manual_seed(3 * t + 10 * b + c)
        a, bb = _rnd(torch.randn(b, c, t, generator=g), act), _rnd(torch.randn(b, c, t, generator=g), act)
        ad, bd = _in_rows(a, p, act), _in_rows(bb, p, act)
        for lens in [None] + _len_sets(b, t):
            ln = None if lens is None else torch.tensor(lens, dtype=torch.int32)
            lnd = None if ln is None else ln.cuda()
            out = _out(b * c, p, DT[act])
            assert L.ts_train_add(ad.data_ptr(), bd.data_ptr(), _ptr(lnd), c, out.data_ptr(), b * c, t, p, act, _stream()) == 0
            torch.cuda.synchronize()
            what = f"add b={b} c={c} t={t} pitch={p} len_b={lens} act={act}"
            ref = a.double() + bb.double() * (1.0 if ln is None else _mask(ln, t))
            _check(out[:-1, :t].view(b, c, t), ref, 2e-5, "add", what, bf16=bool(act))
            _guard_ok(out, what)


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("t", ROW_T)
def test_add_relu_forward_and_relu_backward(t, act):
    """ts_train_add_relu_fwd: relu(a + b), relu(a) when b is NULL; ts_train_relu_bwd on the reference's own rounded output: dout where out > 0, else +0.0"""
    _lib, L = _api()
    for b, c, p in _row_shapes(t):
        g = torch.Generator().manual_seed(5 * t + 10 * b + c)
        rows = b * c
        a, bb, dout = (_rnd(torch.randn(rows, t, generator=g), act) for _ in range(3))
        ad, bd, dd = _in_rows(a, p, act), _in_rows(bb, p, act), _in_rows(dout, p, act)
        for with_b in (True, False):
            what = f"add_relu rows={rows} t={t} pitch={p} b={with_b} act={act}"
            ref = torch.relu(a.double() + (bb.double() if with_b else 0.0))
            out = _out(rows, p, DT[act])
            assert L.ts_train_add_relu_fwd(ad.data_ptr(), _ptr(bd) if with_b else None, out.data_ptr(), rows, t, p, act, _stream()) == 0
            torch.cuda.synchronize()
            _check(out[:-1, :t], ref, 2e-5, "add_relu_fwd", what, bf16=bool(act))
            _guard_ok(out, what)
            o_ref = _rnd(ref, act)                                           # the gate is an input: the reference's own rounded output
            din = _out(rows, p, DT[act])
            assert L.ts_train_relu_bwd(dd.data_ptr(), _keep(_in_rows(o_ref, p, act)), din.data_ptr(), rows, t, p, act, _stream()) == 0
            torch.cuda.synchronize()
            _assert_bits(din[:-1, :t], torch.where(o_ref > 0, dout, torch.zeros_like(dout)), what + " relu_bwd")
            _guard_ok(din, what + " relu_bwd")


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("t", ROW_T)
def test_squeeze_excite_row_passes(t, act):
    """ts_train_se_pool (mean over ALL t frames), ts_train_se_scale (x gate [+ add_mean / t]), ts_train_se_rowdot (sum_t a b)"""
    _lib, L = _api()
    for b, c, p in _row_shapes(t):
        g = torch.Generator().manual_seed(7 * t + 10 * b + c)
        rows = b * c
        x, a2 = _rnd(0.5 + torch.randn(rows, t, generator=g), act), _rnd(torch.randn(rows, t, generator=g), act)
        gate, addm = torch.rand(rows, generator=g), torch.randn(rows, generator=g)
        xd, a2d, gd, amd = _in_rows(x, p, act), _in_rows(a2, p, act), gate.cuda(), addm.cuda()
        what = f"se rows={rows} t={t} pitch={p} act={act}"
        n_round = ((t + 63) // 64 + 9) * U24
        mean = _out(rows, 1)
        assert L.ts_train_se_pool(xd.data_ptr(), mean.data_ptr(), rows, t, p, act, _stream()) == 0
        dot = _out(rows, 1)
        assert L.ts_train_se_rowdot(xd.data_ptr(), a2d.data_ptr(), dot.data_ptr(), rows, t, p, act, _stream()) == 0
        torch.cuda.synchronize()
        for got, terms, div, kind in ((mean, x.double(), t, "se_pool"), (dot, x.double() * a2.double(), 1, "se_rowdot")):
            assert not bool(torch.isnan(got).any()), what + f" {kind}: unwritten or NaN out of the padding"
            _report(kind, what, (got[:-1, 0].double().cpu() - terms.sum(1) / div).abs(), n_round * terms.abs().sum(1) / div)
            _guard_ok(got, what + " " + kind)
        for with_add in (False, True):
            y = _out(rows, p, DT[act])
            assert L.ts_train_se_scale(xd.data_ptr(), gd.data_ptr(), amd.data_ptr() if with_add else None, y.data_ptr(), rows, t, p, act, _stream()) == 0
            torch.cuda.synchronize()
            ref = x.double() * gate.double()[:, None] + (addm.double()[:, None] / t if with_add else 0.0)
            _check(y[:-1, :t], ref, 2e-5, "se_scale", what + f" add_mean={with_add}", bf16=bool(act))
            _guard_ok(y, what + " se_scale")


def _bf16_edge_values():
    """finite values whose rounding to bf16 is decided by the tie rule or sits at an end of the range"""
    e = 2.0 ** -8
    v = [1 + e, 1 + 3 * e, -(1 + e), -(1 + 3 * e), 1 + e + 2.0 ** -20, 1 + e - 2.0 ** -20, -0.0, 0.0, float(torch.finfo(BF).max), -float(torch.finfo(BF).max),
         2.0 ** -126, -(2.0 ** -126), 2.0 ** -126 * (1 + e), 2.0 ** -126 * (1 + 3 * e), 255.5, 256.5 * 2.0 ** -7]
    return torch.tensor(v, dtype=torch.float64).float()


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("t", ROW_T)
def test_act_import_and_export_are_bit_exact(t, act):
    """ts_train_act_import: contiguous f32 [rows][t] -> pitched rows (act 1: round to nearest even); ts_train_act_export: the way back (exact); a round trip"""
    _lib, L = _api()
    edge = _bf16_edge_values()
    for b, c, p in _row_shapes(t):
        g = torch.Generator().manual_seed(11 * t + 10 * b + c)
        rows = b * c
        src = torch.randn(rows * t, generator=g)
        n = min(edge.numel(), rows * t)
        src[:n] = edge[:n]
        src = src.view(rows, t)
        what = f"act_import/export rows={rows} t={t} pitch={p} act={act}"
        dst = _out(rows, p, DT[act])
        assert L.ts_train_act_import(_dev(src), dst.data_ptr(), rows, t, p, act, _stream()) == 0
        torch.cuda.synchronize()
        _assert_bits(dst[:-1, :t], src.to(DT[act]), what + " import")
        _guard_ok(dst, what + " import")
        # export alone, out of rows with NaN in their padding
        held = _rnd(torch.randn(rows, t, generator=g), act)
        held.view(-1)[:n] = _rnd(edge[:n], act)
        back = _out(rows, t)                                                  # contiguous [rows][t]; the guard is one more row of t floats
        assert L.ts_train_act_export(_keep(_in_rows(held, p, act)), back.data_ptr(), rows, t, p, act, _stream()) == 0
        # the round trip: export what the import left (its columns >= t are the import's, not NaN)
        trip = _out(rows, t)
        assert L.ts_train_act_export(dst.data_ptr(), trip.data_ptr(), rows, t, p, act, _stream()) == 0
        torch.cuda.synchronize()
        _assert_bits(back[:-1], held, what + " export")
        _assert_bits(trip[:-1], _rnd(src, act), what + " round trip")
        _guard_ok(back, what + " export")
        _guard_ok(trip, what + " round trip")


@pytest.mark.parametrize("n", [1, 3, 4, 5, 16, 1023, 1024, 1027, 4099])
def test_cast_bf16_rounds_to_nearest_even(n):
    """ts_train_cast_bf16: four elements per thread and a scalar tail"""
    _lib, L = _api()
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g) * torch.exp(8 * torch.randn(n, generator=g))
    edge = _bf16_edge_values()
    m = min(n, edge.numel())
    x[n - m:] = edge[:m]                                                     # the scalar tail meets edge values too
    x[:m] = edge[:m].flip(0)[:m] if n >= 2 * m else x[:m]
    y = torch.full((n + 8,), NAN, dtype=BF, device="cuda")
    y[n:] = GUARD
    assert L.ts_train_cast_bf16(_dev(x), y.data_ptr(), n, _stream()) == 0
    torch.cuda.synchronize()
    _assert_bits(y[:n], x.to(BF), f"cast_bf16 n={n}")
    assert bool((y[n:] == GUARD).all()), f"cast_bf16 n={n}: wrote behind the output"


# ---------------------------------------------------------------------------------------------------------------------
# 2. ts_train_subsample_mask
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("t_in,t_out,stride,lens", [(10, 4, 3, [6, 7, 5, 10, 0, 13, -2]), (1501, 751, 2, [1500, 1501, 1499, 2, 1, 0, 1600]),
                                                     (513, 513, 1, [513, 512, 511, 1, 0, 600, 257])])
def test_subsample_mask_forward_and_backward_are_bit_equal(t_in, t_out, stride, lens, act):
    """forward: y[j] = x[j stride] if j stride < len else 0; backward: dx[i] = dy[i / stride] where the forward read frame i, +0.0 elsewhere.  Lengths on,
    behind and in front of a sampled frame."""
    _lib, L = _api()
    b, c = len(lens), 2
    pin, pout = _r8(t_in) + 64, _r8(t_out)
    g = torch.Generator().manual_seed(t_in)
    x, dy = _rnd(torch.randn(b, c, t_in, generator=g), act), _rnd(torch.randn(b, c, t_out, generator=g), act)
    ln = torch.tensor(lens, dtype=torch.int32)
    lc = ln.long().clamp(0, t_in)
    what = f"subsample_mask t_in={t_in} t_out={t_out} stride={stride} act={act}"
    src = torch.arange(t_out) * stride                                        # the frame output j reads
    read = src[None, :] < lc[:, None]                                         # [b][t_out]
    y = _out(b * c, pout, DT[act])
    assert L.ts_train_subsample_mask(_keep(_in_rows(x, pin, act)), _dev(ln), y.data_ptr(), b, c, t_in, t_out, stride, 0, pin, pout, act,
                                     _stream()) == 0
    dx = _out(b * c, pin, DT[act])
    assert L.ts_train_subsample_mask(_keep(_in_rows(dy, pout, act)), _dev(ln), dx.data_ptr(), b, c, t_in, t_out, stride, 1, pin, pout, act,
                                     _stream()) == 0
    torch.cuda.synchronize()
    want_y = torch.where(read[:, None, :].expand(b, c, t_out), x[:, :, src], torch.zeros(b, c, t_out))
    _assert_bits(y[:-1, :t_out].view(b, c, t_out), want_y, what + " forward")
    want_dx = torch.zeros(b, c, t_in)
    want_dx[:, :, src] = torch.where(read[:, None, :].expand(b, c, t_out), dy, torch.zeros(b, c, t_out))
    _assert_bits(dx[:-1, :t_in].view(b, c, t_in), want_dx, what + " backward")
    _guard_ok(y, what + " forward")
    _guard_ok(dx, what + " backward")
    # an output frame that would read behind the input
    t_bad = (t_in - 1) // stride + 2
    big = torch.zeros(b * c, _r8(t_bad) + pin, dtype=DT[act], device="cuda")
    assert L.ts_train_subsample_mask(big.data_ptr(), _dev(ln), big.data_ptr(), b, c, t_in, t_bad, stride, 0, pin, _r8(t_bad), act,
                                     _stream()) == _lib.TS_EINVAL
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# 3. two-step BatchNorm: what the step runs once batch x ceil(t / 512) exceeds the one-launch tail's 32 (bf16) / 16 (f32) row units
# ---------------------------------------------------------------------------------------------------------------------
def _spread(b, c, t, g, act, mean=3.0, spread=2.0):
    """[b][c][t] with sample mean `mean` and sample deviation `spread` per channel before rounding (E[v^2] / var = 1 + (mean / spread)^2 whatever n is)"""
    z = torch.randn(b, c, t, generator=g, dtype=torch.float64)
    if b * t > 1:
        z = (z - z.mean((0, 2), keepdim=True)) / z.var((0, 2), unbiased=False, keepdim=True).sqrt()
    return _rnd(mean + spread * z, act)


def _stats(v64):
    mu = v64.mean((0, 2))
    return mu, ((v64 - mu[None, :, None]) ** 2).mean((0, 2))


def _bn64(v64, gamma, beta, relu):
    """BatchNorm1d in train mode written out: statistics over all B * T frames, biased variance, eps 1e-3"""
    mu, var = _stats(v64)
    y = (v64 - mu[None, :, None]) / torch.sqrt(var[None, :, None] + EPS) * gamma[None, :, None] + beta[None, :, None]
    return torch.relu(y) if relu else y


def _group_sums(v64):
    """what ts_train_bn_stats leaves: [8][C][2] sums over the clips of group g = clips [g per, (g + 1) per), per = ceil(B / 8)"""
    b, c, _ = v64.shape
    per = (b + 7) // 8
    out, absum = torch.zeros(8, c, 2, dtype=torch.float64), torch.zeros(8, c, 2, dtype=torch.float64)
    for g in range(8):
        part = v64[g * per:min((g + 1) * per, b)]
        out[g, :, 0], out[g, :, 1] = part.sum((0, 2)), (part * part).sum((0, 2))
        absum[g, :, 0], absum[g, :, 1] = part.abs().sum((0, 2)), out[g, :, 1]
    return out, absum


def _check_mean_rstd(mr, v64, what, kind):
    """mr: device f32 [C + 1][2] with its guard row"""
    mu, var = _stats(v64)
    rstd = 1.0 / torch.sqrt(var + EPS)
    ev2 = (v64 * v64).mean((0, 2))
    got = mr[:-1].double().cpu()
    assert not bool(torch.isnan(got).any()), f"{what}: mean_rstd unwritten"
    _report(kind + " mean", what, (got[:, 0] - mu).abs(), 1e-6 * v64.abs().mean((0, 2)) + 2.0 ** -23 * mu.abs())
    # 1e-5 for E[v^2] / var = 3.25 (spread 2 around mean 3); in general 1e-6 x E[v^2] / var, the cancellation of s2 / n - m^2
    rel = torch.where(ev2 / var <= 3.3, torch.full_like(var, 1e-5), 1e-6 * ev2 / var)
    _report(kind + " rstd", what, (got[:, 1] - rstd).abs(), rel * rstd)
    _guard_ok(mr, what + " mean_rstd")


class _Running:
    """running statistics that start from random values, and their reference after one step"""

    def __init__(self, c, g, use=True, counter=True):
        self.rm0, self.rv0 = 0.5 + torch.rand(c, generator=g), 0.5 + torch.rand(c, generator=g)
        self.rm, self.rv = (_start(self.rm0[:, None]), _start(self.rv0[:, None])) if use else (None, None)
        self.nbt = torch.tensor([41, 7], dtype=torch.int64, device="cuda") if use and counter else None

    def ptrs(self):
        return _ptr(self.rm), _ptr(self.rv), 0.1, _ptr(self.nbt)

    def check(self, v64, what, kind):
        if self.rm is None:
            return
        n = v64.shape[0] * v64.shape[2]
        mu, var = _stats(v64)
        for got, ref, name in ((self.rm, 0.9 * self.rm0.double() + 0.1 * mu, "running_mean"), (self.rv, 0.9 * self.rv0.double() + 0.1 * var * n / (n - 1), "running_var")):
            g = got[:-1, 0].double().cpu()
            _report(kind + " running", what + " " + name, (g - ref).abs(), 1e-5 * ref.abs())
            _guard_ok(got, what + " " + name)
        if self.nbt is not None:
            assert self.nbt.tolist() == [42, 7], f"{what}: the counter went from 41 to {self.nbt.tolist()}"


def _bn_case(batch, ch, t, act, mean=3.0):
    _lib, L = _api()
    g = torch.Generator().manual_seed(1000 * batch + 10 * t + ch + act)
    pitch = _r8(t) + (64 if batch % 2 else 0)
    bf = bool(act)
    tag = f"batch={batch} ch={ch} t={t} act={act} mean={mean}"
    v = _spread(batch, ch, t, g, act, mean=mean)
    v64 = v.double()
    vd = _in_rows(v, pitch, act)
    gamma, beta = 1.0 + 0.3 * torch.randn(ch, generator=g), 0.2 * torch.randn(ch, generator=g)
    gd, bd = gamma.cuda(), beta.cuda()
    rows = batch * ch
    # ---- ts_train_bn_stats
    sums = torch.full((8 * ch * 2 + 2,), NAN, dtype=torch.float64, device="cuda")
    sums[-2:] = GUARD
    assert L.ts_train_bn_stats(vd.data_ptr(), sums.data_ptr(), batch, ch, t, pitch, act, _stream()) == 0
    torch.cuda.synchronize()
    ref_s, abs_s = _group_sums(v64)
    got_s = sums[:-2].cpu().view(8, ch, 2)
    assert not bool(torch.isnan(got_s).any()), f"bn_stats {tag}: unwritten sums"
    _report("bn_stats", f"bn_stats {tag}", (got_s - ref_s).abs(), 1e-6 * abs_s)        # an empty group: exactly 0
    assert bool((sums[-2:] == GUARD).all()), f"bn_stats {tag}: wrote behind the sums"
    # ---- ts_train_bn_fwd
    mr_ref = None
    for relu in (0, 1):
        ref_y = _bn64(v64, gamma.double(), beta.double(), relu)
        for use, counter in ((True, True), (True, False), (False, False)):
            run = _Running(ch, g, use, counter)
            y, mr = _out(rows, pitch, DT[act]), _out(ch, 2)
            ws = torch.full((16 * ch,), NAN, dtype=torch.float64, device="cuda")
            assert L.ts_train_bn_fwd(vd.data_ptr(), gd.data_ptr(), bd.data_ptr(), y.data_ptr(), mr.data_ptr(), ws.data_ptr(), batch, ch, t, pitch, EPS, relu,
                                     *run.ptrs(), act, _stream()) == 0
            torch.cuda.synchronize()
            what = f"bn_fwd {tag} relu={relu} running={use} counter={counter}"
            _check(y[:-1, :t].view(batch, ch, t), ref_y, 2e-5, "bn_fwd y", what, bf16=bf)
            _guard_ok(y, what)
            _check_mean_rstd(mr, v64, what, "bn_fwd")
            run.check(v64, what, "bn_fwd")
    # ---- ts_train_bn_bwd: float64 autograd through the written-out BatchNorm; y and mean_rstd are the reference's own, rounded
    mu, var = _stats(v64)
    mr_in = torch.stack([mu, 1.0 / torch.sqrt(var + EPS)], 1).float()
    dy = _rnd(torch.randn(batch, ch, t, generator=g), act)
    dyd = _in_rows(dy, pitch, act)
    for relu in (0, 1):
        leaf = [x.double().requires_grad_(True) for x in (v, gamma, beta)]
        y64 = _bn64(*leaf, relu)
        (y64 * dy.double()).sum().backward()
        yd = _in_rows(_rnd(y64.detach(), act), pitch, act)
        dv, dg, db = _out(rows, pitch, DT[act]), _out(ch, 1), _out(ch, 1)
        ws = torch.full((16 * ch,), NAN, dtype=torch.float64, device="cuda")
        assert L.ts_train_bn_bwd(dyd.data_ptr(), yd.data_ptr(), vd.data_ptr(), gd.data_ptr(), _dev(mr_in), dv.data_ptr(), dg.data_ptr(), db.data_ptr(),
                                 ws.data_ptr(), batch, ch, t, pitch, relu, act, _stream()) == 0
        torch.cuda.synchronize()
        what = f"bn_bwd {tag} relu={relu}"
        # dv = k (g - mean g - xhat mean(g xhat)) cancels (to ~eps / var of g when n = 2): whatever the kernel, its three f32 terms each carry a few
        # roundings of their OWN size, and xhat inherits 2^-24 |mean| rstd from the f32 mean it is handed -- 8 x 2^-24 of the terms' absolute sum
        gate = (y64.detach() > 0).double() if relu else 1.0
        g64 = dy.double() * gate
        xhat = (v64 - mr_in[:, 0].double()[None, :, None]) * mr_in[:, 1].double()[None, :, None]
        kk, mg, mgx = (gamma.double() * mr_in[:, 1].double()).abs()[None, :, None], g64.mean((0, 2)).abs()[None, :, None], (g64 * xhat).mean((0, 2)).abs()[None, :, None]
        cancel = 8 * U24 * kk * (g64.abs() + mg + (xhat.abs() + (mr_in[:, 0].double().abs() * mr_in[:, 1].double())[None, :, None]) * mgx)
        _check(dv[:-1, :t].view(batch, ch, t), leaf[0].grad, 1e-4, "bn_bwd dv", what, bf16=bf, extra=cancel)
        _check(dg[:-1, 0], leaf[1].grad, 1e-4, "bn_bwd dgamma", what + " dgamma")
        _check(db[:-1, 0], leaf[2].grad, 1e-4, "bn_bwd dbeta", what + " dbeta")
        for o in (dv, dg, db):
            _guard_ok(o, what)
        # ---- ts_train_bn_bwd_sums: the second half alone, fed with the reference's g, dgamma, dbeta (what the depthwise backward's epilogue leaves)
        g_in = _rnd(g64, act)
        dgam_in, dbet_in = leaf[1].grad.float(), leaf[2].grad.float()
        n = batch * t
        ref_dv = (gamma.double() * mr_in[:, 1].double())[None, :, None] * (g_in.double() - dbet_in.double()[None, :, None] / n
                                                                         - xhat * dgam_in.double()[None, :, None] / n)
        dv2 = _out(rows, pitch, DT[act])
        assert L.ts_train_bn_bwd_sums(_keep(_in_rows(g_in, pitch, act)), vd.data_ptr(), gd.data_ptr(), _dev(mr_in), _dev(dgam_in),
                                      _dev(dbet_in), dv2.data_ptr(), batch, ch, t, pitch, act, _stream()) == 0
        torch.cuda.synchronize()
        _check(dv2[:-1, :t].view(batch, ch, t), ref_dv, 1e-4, "bn_bwd_sums dv", f"bn_bwd_sums {tag} relu={relu}", bf16=bf, extra=cancel)
        _guard_ok(dv2, f"bn_bwd_sums {tag}")
        if not act:                                                          # f32: g is the autograd's own, so both halves meet the same gradient
            _check(dv2[:-1, :t].view(batch, ch, t), leaf[0].grad, 1e-4, "bn_bwd_sums dv", f"bn_bwd_sums {tag} relu={relu} against autograd", extra=cancel)
    # ---- ts_train_bn2_add_relu_fwd fed by two ts_train_bn_stats
    vb = _spread(batch, ch, t, g, act, mean=-1.0, spread=0.7)
    vbd = _in_rows(vb, pitch, act)
    gamma_b, beta_b = 1.0 + 0.3 * torch.randn(ch, generator=g), 0.2 * torch.randn(ch, generator=g)
    sums_b = torch.full((8 * ch * 2,), NAN, dtype=torch.float64, device="cuda")
    assert L.ts_train_bn_stats(vbd.data_ptr(), sums_b.data_ptr(), batch, ch, t, pitch, act, _stream()) == 0
    ra, rb = _Running(ch, g), _Running(ch, g, True, False)
    out, mra, mrb = _out(rows, pitch, DT[act]), _out(ch, 2), _out(ch, 2)
    assert L.ts_train_bn2_add_relu_fwd(vd.data_ptr(), sums.data_ptr(), gd.data_ptr(), bd.data_ptr(), EPS, mra.data_ptr(), *ra.ptrs(),
                                       vbd.data_ptr(), sums_b.data_ptr(), _dev(gamma_b), _dev(beta_b), EPS, mrb.data_ptr(), *rb.ptrs(),
                                       out.data_ptr(), batch, ch, t, pitch, act, _stream()) == 0
    torch.cuda.synchronize()
    what = f"bn2_add_relu_fwd {tag}"
    ref = torch.relu(_bn64(v64, gamma.double(), beta.double(), 0) + _bn64(vb.double(), gamma_b.double(), beta_b.double(), 0))
    _check(out[:-1, :t].view(batch, ch, t), ref, 2e-5, "bn2_add_relu_fwd out", what, bf16=bf)
    _guard_ok(out, what)
    _check_mean_rstd(mra, v64, what + " a", "bn2_add_relu_fwd")
    _check_mean_rstd(mrb, vb.double(), what + " b", "bn2_add_relu_fwd")
    ra.check(v64, what + " a", "bn2_add_relu_fwd")
    rb.check(vb.double(), what + " b", "bn2_add_relu_fwd")
    return vd, vbd, gd, bd, mra, mrb, out, pitch


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("t", [2, 501, 513, 1030])
@pytest.mark.parametrize("ch", [1, 2, 5])
@pytest.mark.parametrize("batch", [1, 3, 8, 9, 33])                           # the 8 clip groups: some empty, one clip each, uneven
def test_two_step_batchnorm_matches_float64(batch, ch, t, act):
    """ts_train_bn_stats, ts_train_bn_fwd, ts_train_bn_bwd, ts_train_bn_bwd_sums, ts_train_bn2_add_relu_fwd"""
    _bn_case(batch, ch, t, act)


@pytest.mark.parametrize("act", [0, 1])
def test_two_step_batchnorm_with_a_mean_of_fifty_spreads(act):
    """mean 100, spread 2: E[v^2] / var = 2501, so rstd is bound by 1e-6 x 2501 (the cancellation in s2 / n - m^2)"""
    _bn_case(9, 2, 513, act, mean=100.0)


def test_the_one_launch_tail_hands_over_to_the_two_step_kernels():
    """33 clips x 2 channels x 513 frames in bf16 = 66 row units > 32: ts_train_bn2_add_relu_chan_fwd answers TS_EUNSUPPORTED, and the two-step kernels
    (checked against float64 inside _bn_case) take the shape"""
    _lib, L = _api()
    vd, vbd, gd, bd, mra, mrb, out, pitch = _bn_case(33, 2, 513, 1)
    rc = L.ts_train_bn2_add_relu_chan_fwd(vd.data_ptr(), gd.data_ptr(), bd.data_ptr(), EPS, mra.data_ptr(), None, None, 0.1, None, vbd.data_ptr(), gd.data_ptr(),
                                          bd.data_ptr(), EPS, mrb.data_ptr(), None, None, 0.1, None, out.data_ptr(), 33, 2, 513, pitch, 1, _stream())
    assert rc == _lib.TS_EUNSUPPORTED
    assert L.ts_train_bn2_add_relu_chan_fwd(vd.data_ptr(), gd.data_ptr(), bd.data_ptr(), EPS, mra.data_ptr(), None, None, 0.1, None, vbd.data_ptr(), gd.data_ptr(),
                                            bd.data_ptr(), EPS, mrb.data_ptr(), None, None, 0.1, None, out.data_ptr(), 32, 2, 501, pitch, 1, _stream()) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# 4. depthwise forward with the BatchNorm input: pair kernel, matrix-core kernel, per-tile statistics
# ---------------------------------------------------------------------------------------------------------------------
def _len_pat(batch, t, shift):
    pat = [t, 1, 0, t - 1, t // 2 + 1, t + 5]                                 # full, one frame, empty, ragged, beyond the row (the kernels clamp)
    return torch.tensor([pat[(i + shift) % 6] for i in range(batch)], dtype=torch.int32)


def _dw64(x, w, len_in, len_out, stride=1, dil=1, pad=0):
    """the depthwise MaskedConv1d in float64: x zeroed from len_in on, y zeroed from len_out on when given"""
    xm = x if len_in is None else x * _mask(len_in, x.shape[-1])
    y = F.conv1d(xm, w[:, None, :], stride=stride, padding=pad, dilation=dil, groups=x.shape[1])
    return y if len_out is None else y * _mask(len_out, y.shape[-1])


def _sums_device(v64):
    return _group_sums(v64)[0].cuda().contiguous()


def _tile_sums(v64, n_tiles):
    """f32 [C][n_tiles][2]: (sum v, sum v^2) of n_tiles runs of the channel's B * T frames (what a pointwise launch's epilogue leaves)"""
    b, c, t = v64.shape
    flat = v64.permute(1, 0, 2).reshape(c, b * t)
    out = torch.zeros(c, n_tiles, 2, dtype=torch.float64)
    for i, part in enumerate(torch.tensor_split(flat, n_tiles, dim=1)):
        out[:, i, 0], out[:, i, 1] = part.sum(1), (part * part).sum(1)
    return out.float().cuda().contiguous()


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("in_relu", [0, 1])
@pytest.mark.parametrize("t,k", [(37, 5), (501, 33), (520, 75), (1100, 127)])
@pytest.mark.parametrize("batch", [2, 17, 33])
@pytest.mark.parametrize("ch", [2, 6])
def test_depthwise_forward_with_the_batchnorm_input(ch, batch, t, k, in_relu, act):
    """ts_train_dwconv_fwd_bn on the pair kernel (f32 rows; bf16 rows below 17 clips) and on the matrix-core kernel (bf16 rows, >= 17 clips), and
    ts_train_dwconv_fwd_bn_tiles with tile sums formed on the CPU (37 and 70 tiles: no multiple of 64, and more than a wave has lanes): y, the published
    mean_rstd, both running statistics and the counter.  Frames >= len_in enter the convolution as zero, not as BatchNorm(0)."""
    _lib, L = _api()
    g = torch.Generator().manual_seed(10000 * ch + 100 * batch + t + in_relu)
    pad, pitch, rows = (k - 1) // 2, _r8(t) + (64 if in_relu else 0), batch * ch
    mfma = act == 1 and batch >= 17
    v = _spread(batch, ch, t, g, act)
    v64, vd = v.double(), _in_rows(v, pitch, act)
    gamma, beta = 1.0 + 0.3 * torch.randn(ch, generator=g), 0.2 * torch.randn(ch, generator=g)
    w = torch.randn(ch, k, generator=g) / k ** 0.5
    w64 = w.to(BF).double() if mfma else w.double()                           # the matrix-core kernel rounds the taps to bf16
    gd, bd, wd, sums = gamma.cuda(), beta.cuda(), w.cuda(), _sums_device(v64)
    x64 = _bn64(v64, gamma.double(), beta.double(), in_relu)
    for li, lo in ((_len_pat(batch, t, 0), None), (_len_pat(batch, t, 2), _len_pat(batch, t, 4))):
        ref = _dw64(x64, w64, li, lo, pad=pad)
        # matrix cores: x is rounded to bf16 on its way into the MFMA -- up to 2^-8 of every product (see the module docstring)
        extra = 2.0 ** -8 * (1 + 2.0 ** -8) * _dw64(x64.abs(), w64.abs(), li, lo, pad=pad) if mfma else None
        lid, lod = li.cuda(), None if lo is None else lo.cuda()
        for tiles in [0] + ([37, 70] if mfma else []):
            run, y, mr = _Running(ch, g, True, lo is None), _out(rows, pitch, DT[act]), _out(ch, 2)
            tail = (*run.ptrs(), lid.data_ptr(), _ptr(lod), wd.data_ptr(), y.data_ptr(), batch, ch, t, k, pad, pitch, act, _stream())
            if tiles:
                ts = _tile_sums(v64, tiles)
                assert L.ts_train_dwconv_fwd_bn_tiles(vd.data_ptr(), ts.data_ptr(), tiles, gd.data_ptr(), bd.data_ptr(), EPS, in_relu, mr.data_ptr(), *tail) == 0
            else:
                assert L.ts_train_dwconv_fwd_bn(vd.data_ptr(), sums.data_ptr(), gd.data_ptr(), bd.data_ptr(), EPS, in_relu, mr.data_ptr(), *tail) == 0
            torch.cuda.synchronize()
            kind = "dwconv_fwd_bn" + ("_tiles" if tiles else "") + (" mfma" if mfma else " pair")
            what = f"{kind} ch={ch} batch={batch} t={t} k={k} in_relu={in_relu} act={act} len_out={'given' if lo is not None else 'NULL'} tiles={tiles}"
            _check(y[:-1, :t].view(batch, ch, t), ref, 2e-5, kind + " y", what, bf16=bool(act), extra=extra)
            _guard_ok(y, what)
            _check_mean_rstd(mr, v64, what, kind)
            run.check(v64, what, kind)


def test_depthwise_forward_with_a_mean_of_fifty_spreads_publishes_the_statistics():
    """mean 100, spread 2 through ts_train_dwconv_fwd_bn (pair kernel) and _bn_tiles (matrix cores): mean_rstd and the running statistics"""
    _lib, L = _api()
    g = torch.Generator().manual_seed(50)
    batch, ch, t, k, pad = 17, 2, 501, 33, 16
    pitch = _r8(t)
    w = (torch.randn(ch, k, generator=g) / k ** 0.5).cuda()
    gd, bd = torch.ones(ch, device="cuda"), torch.zeros(ch, device="cuda")
    for act in (0, 1):
        v = _spread(batch, ch, t, g, act, mean=100.0)
        vd = _in_rows(v, pitch, act)
        for tiles in [0] + ([37] if act else []):
            run, y, mr = _Running(ch, g), _out(batch * ch, pitch, DT[act]), _out(ch, 2)
            tail = (*run.ptrs(), None, None, w.data_ptr(), y.data_ptr(), batch, ch, t, k, pad, pitch, act, _stream())
            if tiles:
                assert L.ts_train_dwconv_fwd_bn_tiles(vd.data_ptr(), _keep(_tile_sums(v.double(), tiles)), tiles, gd.data_ptr(), bd.data_ptr(), EPS, 1,
                                                      mr.data_ptr(), *tail) == 0
            else:
                assert L.ts_train_dwconv_fwd_bn(vd.data_ptr(), _keep(_sums_device(v.double())), gd.data_ptr(), bd.data_ptr(), EPS, 1, mr.data_ptr(), *tail) == 0
            torch.cuda.synchronize()
            what = f"dwconv_fwd_bn mean 100 act={act} tiles={tiles}"
            _check_mean_rstd(mr, v.double(), what, "dwconv_fwd_bn mean 100")
            run.check(v.double(), what, "dwconv_fwd_bn mean 100")
            assert not bool(torch.isnan(y[:-1, :t].float()).any())
            _guard_ok(y, what)


def test_tile_statistics_entry_point_refuses_what_the_matrix_core_kernel_does_not_take():
    _lib, L = _api()
    ch, t, k, pitch = 2, 64, 5, 64
    z = torch.zeros(17 * ch * pitch, device="cuda")
    one = torch.ones(ch * 4 * 2, device="cuda")
    call = lambda batch, act, c=ch, kk=k: L.ts_train_dwconv_fwd_bn_tiles(z.data_ptr(), one.data_ptr(), 4, one.data_ptr(), one.data_ptr(), EPS, 1, one.data_ptr(), None, None,
                                                                          0.1, None, None, None, one.data_ptr(), z.data_ptr(), batch, c, t, kk, (kk - 1) // 2, pitch, act,
                                                                          _stream())
    assert call(17, 0) == _lib.TS_EUNSUPPORTED                                # f32 rows
    assert call(16, 1) == _lib.TS_EUNSUPPORTED                                # too few clips for the MFMA's N dimension
    assert call(17, 1, kk=4) == _lib.TS_EUNSUPPORTED                          # not the "same" geometry
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# 5. two row pairs per wave in dw_fwd_pair_kernel (>= 32 x CU-count pairs: what every real layer has)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,act,batch,ch,t,k,dil,bn", [
    ("f32", 0, 32, 512, 72, 11, 1, False), ("f32", 0, 32, 512, 72, 11, 1, True),
    ("bf16", 1, 16, 1024, 72, 11, 1, False), ("bf16", 1, 16, 1024, 72, 11, 1, True),
    ("last wave owns one pair", 0, 3, 5462, 16, 5, 1, False), ("last wave owns one pair", 0, 3, 5462, 16, 5, 1, True),
    ("phase split", 0, 32, 512, 80, 13, 2, False)])
def test_two_pairs_per_wave_of_the_pair_forward(name, act, batch, ch, t, k, dil, bn):
    _lib, L = _api()
    items = batch * ch // (1 if dil == 2 else 2)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert items >= 32 * cus, f"{items} wave items do not reach the two-per-wave branch on {cus} compute units"
    g = torch.Generator().manual_seed(batch + ch + t)
    pad, pitch, rows = dil * (k - 1) // 2, _r8(t), batch * ch
    v = _spread(batch, ch, t, g, act) if bn else _rnd(torch.randn(batch, ch, t, generator=g), act)
    vd = _in_rows(v, pitch, act)
    w = torch.randn(ch, k, generator=g) / k ** 0.5
    li, lo = _len_pat(batch, t, 0), _len_pat(batch, t, 3)
    y = _out(rows, pitch, DT[act])
    what = f"two pairs per wave: {name} bn={bn}"
    if bn:
        gamma, beta = 1.0 + 0.3 * torch.randn(ch, generator=g), 0.2 * torch.randn(ch, generator=g)
        run, mr = _Running(ch, g), _out(ch, 2)
        assert L.ts_train_dwconv_fwd_bn(vd.data_ptr(), _keep(_sums_device(v.double())), _dev(gamma), _dev(beta), EPS, 1, mr.data_ptr(),
                                        *run.ptrs(), _dev(li), _dev(lo), _dev(w), y.data_ptr(), batch, ch, t, k, pad, pitch, act,
                                        _stream()) == 0
        x64 = _bn64(v.double(), gamma.double(), beta.double(), 1)
    else:
        assert L.ts_train_dwconv_fwd(vd.data_ptr(), _dev(li), _dev(lo), _dev(w), y.data_ptr(), batch, ch, t, t, k, 1, dil, pad,
                                     pitch, pitch, act, _stream()) == 0
        x64 = v.double()
    torch.cuda.synchronize()
    _check(y[:-1, :t].view(batch, ch, t), _dw64(x64, w.double(), li, lo, dil=dil, pad=pad), 2e-5, "dw_fwd_pair two pairs per wave", what, bf16=bool(act))
    _guard_ok(y, what)
    if bn:
        _check_mean_rstd(mr, v.double(), what, "dw_fwd_pair two pairs per wave")
        run.check(v.double(), what, "dw_fwd_pair two pairs per wave")


# ---------------------------------------------------------------------------------------------------------------------
# 6. ts_train_dwconv_bwd_bn on the pair kernel (6 channels: no matrix-core path)
# ---------------------------------------------------------------------------------------------------------------------
def _gate_safe(v, sc, hs, act, g):
    """v with no float64 pre-activation v sc + hs within 1e-4 of zero: the offending elements are drawn again (and rounded again)"""
    for _ in range(50):
        bad = (v.double() * sc[None, :, None] + hs[None, :, None]).abs() < 1e-4
        if not bool(bad.any()):
            return v
        v = torch.where(bad, _rnd(3.0 + 2.0 * torch.randn(v.shape, generator=g), act), v)
    raise AssertionError("could not move the pre-activations away from zero")


def _dw_bwd_bn_ref(v, mr, gamma, beta, in_relu, w64, li, lo, dy, pad):
    """float64 autograd through relu?(gamma xhat + beta) mask -> conv1d, xhat = (v - mean) rstd from the f32 mean_rstd the kernel is handed"""
    xhat = (v.double() - mr[:, 0].double()[None, :, None]) * mr[:, 1].double()[None, :, None]
    gm, bt, wl = gamma.double().requires_grad_(True), beta.double().requires_grad_(True), w64.clone().requires_grad_(True)
    pre = gm[None, :, None] * xhat + bt[None, :, None]
    pre.retain_grad()
    x = torch.relu(pre) if in_relu else pre
    (_dw64(x, wl, li, lo, pad=pad) * dy.double()).sum().backward()
    # sum |dy| |x| per tap: what a relative rounding of every staged x moves dw by at most (the matrix-core backward stages x as bf16)
    w0 = torch.zeros_like(w64).requires_grad_(True)
    (_dw64(x.detach().abs(), w0, li, lo, pad=pad) * dy.double().abs()).sum().backward()
    return dict(g=pre.grad, dw=wl.grad, dgamma=gm.grad, dbeta=bt.grad, pre=pre.detach(), dw_abs=w0.grad)


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("in_relu", [0, 1])
@pytest.mark.parametrize("t,k", [(300, 33), (1030, 75)])
@pytest.mark.parametrize("batch", [3, 16, 33])                                # one, one and three clips per wave
def test_depthwise_backward_with_the_batchnorm_input_on_the_pair_kernel(batch, t, k, in_relu, act):
    """g = dL/dx relu'(v sc + hs) mask, dw, in_dgamma, in_dbeta (the last three ACCUMULATE onto random values: the increment is asserted); dw == NULL"""
    _lib, L = _api()
    ch, pad, pitch, rows = 6, (k - 1) // 2, _r8(t) + 64, batch * 6
    g = torch.Generator().manual_seed(100 * batch + t + in_relu + 7 * act)
    v = _spread(batch, ch, t, g, act)
    mu, var = _stats(v.double())
    mr = torch.stack([mu, 1.0 / torch.sqrt(var + EPS)], 1).float()
    gamma, beta = 1.0 + 0.3 * torch.randn(ch, generator=g), 0.2 * torch.randn(ch, generator=g)
    sc = gamma.double() * mr[:, 1].double()
    hs = beta.double() - mr[:, 0].double() * sc
    if in_relu:
        v = _gate_safe(v, sc, hs, act, g)
    w = torch.randn(ch, k, generator=g) / k ** 0.5
    dy = _rnd(torch.randn(batch, ch, t, generator=g), act)
    li, lo = _len_pat(batch, t, 0), _len_pat(batch, t, 3)
    ref = _dw_bwd_bn_ref(v, mr, gamma, beta, in_relu, w.double(), li, lo, dy, pad)
    if in_relu:
        assert float(ref["pre"].abs().min()) >= 1e-4                         # asserted on the CPU, before the launch
        assert 0.05 < float((ref["pre"] > 0).double().mean()) < 0.95         # and the gate does cut
    vd, dyd = _in_rows(v, pitch, act), _in_rows(dy, pitch, act)
    start = [torch.randn(ch, k, generator=g), torch.randn(ch, 1, generator=g), torch.randn(ch, 1, generator=g)]
    for with_dw in (True, False):
        gout, dw, dgam, dbet = _out(rows, pitch, DT[act]), _start(start[0]), _start(start[1]), _start(start[2])
        assert L.ts_train_dwconv_bwd_bn(dyd.data_ptr(), vd.data_ptr(), _dev(mr), _dev(gamma), _dev(beta), in_relu,
                                        _dev(li), _dev(lo), _dev(w), gout.data_ptr(), dw.data_ptr() if with_dw else None,
                                        dgam.data_ptr(), dbet.data_ptr(), batch, ch, t, k, pad, pitch, act, _stream()) == 0
        torch.cuda.synchronize()
        what = f"dwconv_bwd_bn pair batch={batch} t={t} k={k} in_relu={in_relu} act={act} dw={'given' if with_dw else 'NULL'}"
        _check(gout[:-1, :t].view(batch, ch, t), ref["g"], 1e-4, "dwconv_bwd_bn pair g", what, bf16=bool(act))
        sums_rel = 4e-3 if act else 1e-4
        _check(dgam[:-1, 0].double().cpu() - start[1][:, 0].double(), ref["dgamma"], sums_rel, f"dwconv_bwd_bn pair in_dgamma act {act}", what + " in_dgamma")
        _check(dbet[:-1, 0].double().cpu() - start[2][:, 0].double(), ref["dbeta"], sums_rel, f"dwconv_bwd_bn pair in_dbeta act {act}", what + " in_dbeta")
        if with_dw:
            _check(dw[:-1].double().cpu() - start[0].double(), ref["dw"], 1e-4, "dwconv_bwd_bn pair dw", what + " dw")
        else:
            _assert_bits(dw[:-1], start[0], what + ": dw was not asked for")
        for o in (gout, dw, dgam, dbet):
            _guard_ok(o, what)


# ---------------------------------------------------------------------------------------------------------------------
# 7. general-geometry depthwise kernels (dw_fwd_kernel, dw_bwd_data_kernel, dw_bwd_weight_kernel)
# ---------------------------------------------------------------------------------------------------------------------
GEOMETRIES = {                                                               # channels, t_in, k, stride, dilation, padding
    "stride 2 across the 1024-frame tile": (5, 2100, 33, 2, 1, 16),
    "dilation 3": (4, 300, 13, 1, 3, 18),
    "even k": (2, 300, 4, 1, 1, 2),
    "odd channels, same geometry": (3, 1030, 33, 1, 1, 16),
}


def _t_out(t_in, k, stride, dil, pad):
    return (t_in + 2 * pad - dil * (k - 1) - 1) // stride + 1


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("batch", [1, 9])                                     # the weight gradient splits the clips over <= 8 groups
@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_general_geometry_depthwise_forward_and_gradients(name, batch, act):
    _lib, L = _api()
    ch, t_in, k, stride, dil, pad = GEOMETRIES[name]
    t_out = _t_out(t_in, k, stride, dil, pad)
    assert {"stride 2 across the 1024-frame tile": 1050, "even k": 301}.get(name, t_in) == t_out
    pin, pout = _r8(t_in) + 64, _r8(t_out)
    g = torch.Generator().manual_seed(t_in + batch + k)
    x, dy = _rnd(torch.randn(batch, ch, t_in, generator=g), act), _rnd(torch.randn(batch, ch, t_out, generator=g), act)
    w = torch.randn(ch, k, generator=g) / k ** 0.5
    li, lo = _len_pat(batch, t_in, 0 if batch == 1 else 3), _len_pat(batch, t_out, 0 if batch == 1 else 4)
    xl, wl = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y64 = _dw64(xl, wl, li, lo, stride, dil, pad)
    (y64 * dy.double()).sum().backward()
    xd, dyd, wd, lid, lod = _in_rows(x, pin, act), _in_rows(dy, pout, act), w.cuda(), li.cuda(), lo.cuda()
    what = f"general depthwise: {name} batch={batch} act={act}"
    geo = (batch, ch, t_in, t_out, k, stride, dil, pad, pin, pout, act, _stream())
    y = _out(batch * ch, pout, DT[act])
    assert L.ts_train_dwconv_fwd(xd.data_ptr(), lid.data_ptr(), lod.data_ptr(), wd.data_ptr(), y.data_ptr(), *geo) == 0
    torch.cuda.synchronize()
    _check(y[:-1, :t_out].view(batch, ch, t_out), y64, 2e-5, "dw general fwd", what + " y", bf16=bool(act))
    _guard_ok(y, what + " y")
    start = torch.randn(ch, k, generator=g)
    for with_dx, with_dw in ((True, True), (False, True), (True, False)):
        dx, dw = _out(batch * ch, pin, DT[act]), _start(start)
        assert L.ts_train_dwconv_bwd(dyd.data_ptr(), xd.data_ptr(), lid.data_ptr(), lod.data_ptr(), wd.data_ptr(), dx.data_ptr() if with_dx else None,
                                     dw.data_ptr() if with_dw else None, *geo) == 0
        torch.cuda.synchronize()
        tag = what + f" dx={'given' if with_dx else 'NULL'} dw={'given' if with_dw else 'NULL'}"
        if with_dx:
            _check(dx[:-1, :t_in].view(batch, ch, t_in), xl.grad, 1e-4, "dw general dx", tag + " dx", bf16=bool(act))
        else:
            assert bool(torch.isnan(dx[:-1].float()).all()), tag
        if with_dw:
            _check(dw[:-1].double().cpu() - start.double(), wl.grad, 1e-4, "dw general dw", tag + " dw")
        else:
            _assert_bits(dw[:-1], start, tag + ": dw was not asked for")
        _guard_ok(dx, tag)
        _guard_ok(dw, tag)


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("t", [200, 201, 1032])                              # t = pitch = 8 (mod 16); an odd t; the same behind a second 1024-frame tile
def test_phase_split_rows_on_a_pitch_that_is_no_multiple_of_16(t, act):
    """dilation 2, k 13, padding 12 on the smallest pitch the header allows (round_up(t, 8)): a lane of the phase-split kernels owns 16 frames, and the
    second 8 of a row's last 16 may lie behind the pitch -- in the next row, or behind the tensor.  Forward, dx and dw against float64; full lengths, so
    that every row's first 8 frames are non-zero and a stray store of zeros shows there as well as in the guard row"""
    _lib, L = _api()
    batch, ch, k, dil, pad, pitch = 2, 3, 13, 2, 12, _r8(t)
    g = torch.Generator().manual_seed(t + act)
    x, dy = _rnd(torch.randn(batch, ch, t, generator=g), act), _rnd(torch.randn(batch, ch, t, generator=g), act)
    w = torch.randn(ch, k, generator=g) / k ** 0.5
    xl, wl = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y64 = _dw64(xl, wl, None, None, 1, dil, pad)
    (y64 * dy.double()).sum().backward()
    xd, dyd, wd = _in_rows(x, pitch, act), _in_rows(dy, pitch, act), w.cuda()
    geo = (batch, ch, t, t, k, 1, dil, pad, pitch, pitch, act, _stream())
    what = f"phase split on pitch {pitch}: t={t} act={act}"
    y, dx, dw = _out(batch * ch, pitch, DT[act]), _out(batch * ch, pitch, DT[act]), _start(torch.zeros(ch, k))
    assert L.ts_train_dwconv_fwd(xd.data_ptr(), None, None, wd.data_ptr(), y.data_ptr(), *geo) == 0
    assert L.ts_train_dwconv_bwd(dyd.data_ptr(), xd.data_ptr(), None, None, wd.data_ptr(), dx.data_ptr(), dw.data_ptr(), *geo) == 0
    torch.cuda.synchronize()
    _check(y[:-1, :t].view(batch, ch, t), y64, 2e-5, "dw phase split fwd, pitch 8 mod 16", what + " y", bf16=bool(act))
    _check(dx[:-1, :t].view(batch, ch, t), xl.grad, 1e-4, "dw phase split dx, pitch 8 mod 16", what + " dx", bf16=bool(act))
    _check(dw[:-1], wl.grad, 1e-4, "dw phase split dw, pitch 8 mod 16", what + " dw")
    for o in (y, dx, dw):
        _guard_ok(o, what)


def test_depthwise_entry_points_refuse_what_no_kernel_takes():
    """only the return codes are looked at: every refusal comes before a launch"""
    _lib, L = _api()
    buf = torch.zeros(3 * 8064 + 64, device="cuda")
    w = torch.zeros(3 * 129, device="cuda")
    p, st = buf.data_ptr(), _stream()
    # a fused ("same", even channel count) geometry forms both gradients in one pass and wants dx
    assert L.ts_train_dwconv_bwd(p, p, None, None, w.data_ptr(), None, w.data_ptr(), 1, 2, 300, 300, 11, 1, 1, 5, 304, 304, 0, st) == _lib.TS_EINVAL
    assert L.ts_train_dwconv_bwd(p, p, None, None, w.data_ptr(), None, w.data_ptr(), 1, 3, 300, 300, 13, 1, 2, 12, 304, 304, 0, st) == _lib.TS_EINVAL   # phase split
    # more taps than the kernels cache
    assert L.ts_train_dwconv_fwd(p, None, None, w.data_ptr(), p, 1, 2, 300, 300, 129, 1, 1, 64, 304, 304, 0, st) == _lib.TS_EUNSUPPORTED
    assert L.ts_train_dwconv_bwd(p, p, None, None, w.data_ptr(), p, w.data_ptr(), 1, 2, 300, 300, 129, 1, 1, 64, 304, 304, 0, st) == _lib.TS_EUNSUPPORTED
    # a row too long for the weight-gradient kernel's LDS (the general kernels: 3 channels)
    assert L.ts_train_dwconv_bwd(p, p, None, None, w.data_ptr(), p, w.data_ptr(), 1, 3, 8000, 8000, 33, 1, 1, 16, 8064, 8064, 0, st) == _lib.TS_EUNSUPPORTED
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# 8. deterministic mode: per-workgroup partials in a workspace, summed in workgroup order by a second launch
# ---------------------------------------------------------------------------------------------------------------------
DET_CASES = {                                                                # act, batch, channels, t_in, k, stride, dilation, padding, folded BatchNorm
    "pair": (0, 5, 6, 300, 33, 1, 1, 16, True),
    "phase split": (0, 5, 3, 200, 13, 1, 2, 12, False),
    "general": (0, 9, 5, 401, 33, 2, 1, 16, False),
    "matrix cores": (1, 4, 16, 300, 33, 1, 1, 16, True),
}


@pytest.mark.parametrize("name", sorted(DET_CASES))
def test_deterministic_mode_gives_the_same_bits_twice_and_the_float64_gradients(name):
    _lib, L = _api()
    act, batch, ch, t_in, k, stride, dil, pad, bn = DET_CASES[name]
    mfma = name == "matrix cores"
    t_out = _t_out(t_in, k, stride, dil, pad)
    pin = _r8(t_in)
    pout = pin if stride == 1 else _r8(t_out) + 8
    g = torch.Generator().manual_seed(len(name))
    x = _spread(batch, ch, t_in, g, act) if bn else _rnd(torch.randn(batch, ch, t_in, generator=g), act)
    dy = _rnd(torch.randn(batch, ch, t_out, generator=g), act)
    w = torch.randn(ch, k, generator=g) / k ** 0.5
    w64 = w.to(BF).double() if mfma else w.double()
    li, lo = _len_pat(batch, t_in, 3), _len_pat(batch, t_out, 0)
    if bn:
        mu, var = _stats(x.double())
        mr = torch.stack([mu, 1.0 / torch.sqrt(var + EPS)], 1).float()
        gamma, beta = 1.0 + 0.3 * torch.randn(ch, generator=g), 0.2 * torch.randn(ch, generator=g)
        sc = gamma.double() * mr[:, 1].double()
        x = _gate_safe(x, sc, beta.double() - mr[:, 0].double() * sc, act, g)
        ref = _dw_bwd_bn_ref(x, mr, gamma, beta, 1, w64, li, lo, dy, pad)
        assert float(ref["pre"].abs().min()) >= 1e-4
    else:
        xl, wl = x.double().requires_grad_(True), w64.clone().requires_grad_(True)
        (_dw64(xl, wl, li, lo, stride, dil, pad) * dy.double()).sum().backward()
        ref = dict(g=xl.grad, dw=wl.grad)
    xd, dyd, lid, lod, wd = _in_rows(x, pin, act), _in_rows(dy, pout, act), li.cuda(), lo.cuda(), w.cuda()
    start = [torch.randn(ch, k, generator=g), torch.randn(ch, 1, generator=g), torch.randn(ch, 1, generator=g)]
    ws = torch.full((1 << 18,), NAN, device="cuda")
    runs = []
    try:
        assert L.ts_train_set_deterministic(ws.data_ptr(), ws.numel()) == 0
        for _ in range(2):
            dx, dw, dgam, dbet = _out(batch * ch, pin, DT[act]), _start(start[0]), _start(start[1]), _start(start[2])
            if bn:
                rc = L.ts_train_dwconv_bwd_bn(dyd.data_ptr(), xd.data_ptr(), _dev(mr), _dev(gamma), _dev(beta), 1, lid.data_ptr(),
                                              lod.data_ptr(), wd.data_ptr(), dx.data_ptr(), dw.data_ptr(), dgam.data_ptr(), dbet.data_ptr(), batch, ch, t_in, k, pad,
                                              pin, act, _stream())
            else:
                rc = L.ts_train_dwconv_bwd(dyd.data_ptr(), xd.data_ptr(), lid.data_ptr(), lod.data_ptr(), wd.data_ptr(), dx.data_ptr(), dw.data_ptr(), batch, ch, t_in,
                                           t_out, k, stride, dil, pad, pin, pout, act, _stream())
            assert rc == 0
            torch.cuda.synchronize()
            runs.append((dx, dw, dgam, dbet))
    finally:
        assert L.ts_train_set_deterministic(None, 0) == 0
    for a, b in zip(*runs):
        assert torch.equal(_bits(a.float().cpu()), _bits(b.float().cpu())), f"deterministic mode, {name}: two runs differ"
        _guard_ok(a, f"deterministic mode, {name}")
    dx, dw, dgam, dbet = runs[0]
    what = f"deterministic mode, {name}"
    rel = dict(g=6e-3, dw=1e-5, sums=4e-3) if mfma else dict(g=1e-4, dw=1e-4, sums=1e-4)       # matrix cores: test_gpu_dw_bwd_mfma.py's own bounds
    _check(dx[:-1, :t_in].view(batch, ch, t_in), ref["g"], rel["g"], "deterministic " + name + " dx", what + " dx", bf16=bool(act) and not mfma)
    # matrix cores: the normalised x is staged as bf16, up to 2^-8 of every product dy x (the same derived term as in the forward)
    _check(dw[:-1].double().cpu() - start[0].double(), ref["dw"], rel["dw"], "deterministic " + name + " dw", what + " dw",
           extra=2.0 ** -8 * ref["dw_abs"] if mfma else None)
    if bn:
        _check(dgam[:-1, 0].double().cpu() - start[1][:, 0].double(), ref["dgamma"], rel["sums"], "deterministic " + name + " in_dgamma", what + " in_dgamma")
        _check(dbet[:-1, 0].double().cpu() - start[2][:, 0].double(), ref["dbeta"], rel["sums"], "deterministic " + name + " in_dbeta", what + " in_dbeta")


def test_deterministic_mode_refuses_a_workspace_one_float_too_small():
    """pair kernel, 5 clips: one clip per wave, ceil(5 / 4) = 2 workgroup rows x 6 channels x (k + 2) floats; general kernels, 9 clips: 8 rows"""
    _lib, L = _api()
    st = _stream()
    ws = torch.zeros(8 * 5 * 35, device="cuda")
    buf = lambda *s: torch.zeros(*s, device="cuda")
    x, dy, dx, w, dw = buf(9, 6, 304), buf(9, 6, 304), buf(9, 6, 304), buf(6, 33), buf(6, 33)
    pair = lambda: L.ts_train_dwconv_bwd(dy.data_ptr(), x.data_ptr(), None, None, w.data_ptr(), dx.data_ptr(), dw.data_ptr(), 5, 6, 300, 300, 33, 1, 1, 16, 304, 304, 0, st)
    general = lambda: L.ts_train_dwconv_bwd(dy.data_ptr(), x.data_ptr(), None, None, w.data_ptr(), dx.data_ptr(), dw.data_ptr(), 9, 5, 300, 150, 33, 2, 1, 16, 304, 304, 0, st)
    try:
        assert L.ts_train_set_deterministic(ws.data_ptr(), 2 * 6 * 35 - 1) == 0
        assert pair() == _lib.TS_EINVAL
        assert L.ts_train_set_deterministic(ws.data_ptr(), 2 * 6 * 35) == 0
        assert pair() == 0
        assert L.ts_train_set_deterministic(ws.data_ptr(), 8 * 5 * 35 - 1) == 0
        assert general() == _lib.TS_EINVAL
        assert L.ts_train_set_deterministic(ws.data_ptr(), 8 * 5 * 35) == 0
        assert general() == 0
        assert L.ts_train_set_deterministic(ws.data_ptr(), 0) == _lib.TS_EINVAL
    finally:
        assert L.ts_train_set_deterministic(None, 0) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# 9. pointwise products
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [0, 1, 2])
def test_pointwise_products_match_float64(precision):
    """ts_train_pwconv_fwd / _bwd: v = W u, du = W^T dv, dW = sum over the clips of dv u^T (written, not accumulated).  precision 0: f32; 1: bf16 operands, f32
    results; 2: bf16 results as well"""
    _lib, L = _api()
    batch, c_in, c_out, t, pitch = 3, 24, 40, 77, 136
    g = torch.Generator().manual_seed(precision)
    op, res = int(precision > 0), int(precision == 2)                       # element types of the operands / of the results
    u, dv = _rnd(torch.randn(batch, c_in, t, generator=g), op), _rnd(torch.randn(batch, c_out, t, generator=g), op)
    w = torch.randn(c_out, c_in, generator=g) / c_in ** 0.5
    ud, dvd = _in_rows(u, pitch, op), _in_rows(dv, pitch, op)
    if op:
        wd = torch.full((c_out * c_in + 8,), NAN, dtype=BF, device="cuda")
        assert L.ts_train_cast_bf16(_dev(w), wd.data_ptr(), c_out * c_in, _stream()) == 0
        w64 = w.to(BF).double()
    else:
        wd, w64 = w.cuda(), w.double()
    v, du, dw = _out(batch * c_out, pitch, DT[res]), _out(batch * c_in, pitch, DT[res]), _out(c_out, c_in)
    ws = torch.full((batch * c_out * c_in,), NAN, device="cuda")
    assert L.ts_train_pwconv_fwd(ud.data_ptr(), wd.data_ptr(), v.data_ptr(), batch, c_in, c_out, t, pitch, pitch, precision, _stream()) == 0
    assert L.ts_train_pwconv_bwd(dvd.data_ptr(), ud.data_ptr(), wd.data_ptr(), du.data_ptr(), dw.data_ptr(), ws.data_ptr(), batch, c_in, c_out, t, pitch, pitch,
                                 precision, _stream()) == 0
    torch.cuda.synchronize()
    what = f"pwconv precision={precision}"
    rel_v, rel_du, rel_dw = {0: (2e-5, 1e-4, 1e-4), 1: (2e-3, 2e-3, 2e-3), 2: (6e-3, 6e-3, 2e-3)}[precision]
    _check(v[:-1, :t].view(batch, c_out, t), torch.einsum("oc,bct->bot", w64, u.double()), rel_v, f"pwconv_fwd precision {precision}", what + " v")
    _check(du[:-1, :t].view(batch, c_in, t), torch.einsum("oc,bot->bct", w64, dv.double()), rel_du, f"pwconv_bwd du precision {precision}", what + " du")
    _check(dw[:-1], torch.einsum("bot,bct->oc", dv.double(), u.double()), rel_dw, f"pwconv_bwd dw precision {precision}", what + " dw")
    for o in (v, du, dw):
        _guard_ok(o, what)
    assert L.ts_train_pwconv_fwd(ud.data_ptr(), wd.data_ptr(), v.data_ptr(), batch, c_in, c_out, t, pitch, pitch, 3, _stream()) == _lib.TS_EUNSUPPORTED
