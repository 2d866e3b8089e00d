"""The MXFP8 kernels of csrc/mxfp8.hip through the C ABI of include_staged/thunder_speech_amd/mxfp8.h, against tests/mxfp8_restatement.py and float64.

Conventions (those of tests/test_gpu_gemm_kernels.py): every output buffer has a pitch larger than its row and extra rows behind the last one,
pre-filled with a sentinel no kernel produces (f32 / bf16: a NaN pattern; element bytes: 0x7F, the e4m3fn NaN; scale bytes: 0xFF) -- after the call
everything outside [0, rows) x [0, n) is still the sentinel; operand padding holds NaN (0x7F / 0xFF for MX operands).

1. lane map and packing, exact: integer operands |v| <= 8 that e4m3 holds exactly, scale bytes 125 .. 129 that differ between neighbouring blocks,
   rows and columns, integer bias and residual -- every f32 partial sum is an integer multiple of 2^-4 below 2^20, so the comparison is
   torch.equal with the float64 product of the dequantised operands.  The GELU row is exact at the MX-pair level only (as in 3).
2. ts_mx_quantize_rows: elements and scale bytes bit-equal to the restatement, bf16 and f32 sources, the hand-made blocks of the host test.
3. ts_mx_layernorm_fwd and the GELU -> MX epilogue: the stored f32 result inside the bound of the f32 kernels (1e-5 x max |reference| for the
   LayerNorm, the GELU bound of the bf16 GEMM for the epilogue), the stored MX pair bit-equal to the quantiser of the STORED f32 values.
4. ts_mx_gemm_nt on random operands, element by element: the float64 product of the dequantised values the kernel reads, bound
   E = C_ACC g(k) sum|a b| and the bias / GELU / residual / bf16 terms of test_gpu_gemm_kernels._nt_reference.  C_ACC = 1 would hold for one
   rounding per f32 addition in any order; the instruction does not sum its 128 products that way.  Measured on an MI355X against the float64
   product (bias-free accumulating epilogue onto zeros), worst error / (g(k) sum|a b|) per shape:
       K = 128:  2.61, 2.80, 1.75, 2.42      K = 1024:  0.054, 0.058, 0.057, 0.062      (K = 512: 0.20, K = 4096: 0.006, M = 300, N = 160)
   i.e. a worst error of 2^-15.5 sum|a b| for ONE instruction (K = 128) that falls with the number of instructions summed (2^-17.4, 2^-18.0,
   2^-19.3 at K = 512, 1024, 4096): each instruction's sum of 128 products carries an error of its own, independent from step to step, and the f32
   accumulation across steps adds next to nothing.  The operand maps are not the cause: the exact-integer cases above (partial sums below 2^20 in
   units of 2^-4, every product exact) are bit-equal for every shape and epilogue.  "Twice the worst measured" would be 5.6, above 4, the mark
   beyond which a cause other than the summation order has to be looked for.  What the figures point to is the instruction's internal sum (a
   limited alignment window) -- an inference from the two observations above, not something shown directly.  The test therefore runs at
   C_ACC = 4, the mark itself: worst measured 2.80, a margin of 1.4 x instead of 2 x over these seeded cases (profiles/mxfp8_forward.md).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import test_gpu_gemm_kernels as G
from mxfp8_restatement import handmade_blocks, mx_dequantize, mx_quantize

gpu = pytest.mark.gpu

R, C = 128, 128                                   # TS_MX_GEMM_TILE_ROWS / _COLS (asserted against the header below)
EP_BF16, EP_ACCUM, EP_GELU_MX = 0, 1, 2
SQ, SS = 0x7F, 0xFF                               # sentinels / padding of element and scale bytes
C_ACC = 4.0                                       # the factor c of test 4: worst measured 2.80 (module docstring)
U32 = G.U32
BF = torch.bfloat16


def _api():
    from thunder_speech_amd import _lib
    return _lib, _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bytes(rows, pitch, fill):
    return torch.full((rows, pitch), fill, dtype=torch.uint8, device="cuda")


def _padded_bytes(t, pitch, fill, rows=None):
    out = _bytes(rows or t.shape[0], pitch, fill)
    out[:t.shape[0], :t.shape[1]] = t.cuda()
    return out


def _assert_bytes_outside(buf, m, n, fill, what):
    assert bool((buf[m:] == fill).all()), f"{what}: rows at and beyond M were written"
    assert bool((buf[:m, n:] == fill).all()), f"{what}: columns in [n, pitch) were written"


def _pack(L, wq, ws, n, k):
    """The MX operand of a weight, pitched and padded with NaN bytes, through ts_mx_pack_w."""
    ldq, lds = k + 16, k // 32 + 5
    dq, ds = _padded_bytes(wq, ldq, SQ), _padded_bytes(ws, lds, SS)
    nbytes = L.ts_mx_pack_w_scale_bytes(n, k)
    assert nbytes == (n + 63) // 64 * (k // 128) * 256
    frag, sfrag = torch.full((n * k,), SQ, dtype=torch.uint8, device="cuda"), torch.full((nbytes,), SS, dtype=torch.uint8, device="cuda")
    assert L.ts_mx_pack_w(dq.data_ptr(), ldq, ds.data_ptr(), lds, n, k, frag.data_ptr(), sfrag.data_ptr(), _stream()) == 0
    return frag, sfrag


def _run(inp, ep, use_bias, want_y=True):
    """One product over the MX operands of `inp`; returns the pitched output buffers (y, y16, yq, ys), sentinel-checked."""
    _lib, L = _api()
    d = _lib.STAGED["mxfp8"].defines
    assert (d["TS_MX_GEMM_TILE_ROWS"], d["TS_MX_GEMM_TILE_COLS"]) == (R, C)
    assert (d["TS_MX_EP_BF16"], d["TS_MX_EP_ACCUM"], d["TS_MX_EP_GELU_MX"]) == (EP_BF16, EP_ACCUM, EP_GELU_MX)
    m, n, k = inp["m"], inp["n"], inp["k"]
    ldxq, ldxs = k + 32, k // 32 + 4
    xq, xs = _padded_bytes(inp["xq"], ldxq, SQ), _padded_bytes(inp["xs"], ldxs, SS)
    frag, sfrag = _pack(L, inp["wq"], inp["ws"], n, k)
    bias = inp["bias"].cuda() if use_bias else None
    ldc, ld16, ldyq, ldys = n + 12, n + 24, n + 8, n // 32 + 3
    y = y16 = yq = ys = None
    if ep == EP_BF16:
        y16 = G._sentinel(m + 5, ld16, BF)
    elif ep == EP_ACCUM:
        y = G._sentinel(m + 3, ldc, torch.float32)
        y[:m, :n] = inp["res"].cuda()
    else:
        y = G._sentinel(m + 3, ldc, torch.float32) if want_y else None
        yq, ys = _bytes(m + 2, ldyq, SQ), _bytes(m + 4, ldys, SS)
    ptr = lambda t: None if t is None else t.data_ptr()
    st = L.ts_mx_gemm_nt(xq.data_ptr(), ldxq, xs.data_ptr(), ldxs, frag.data_ptr(), sfrag.data_ptr(), ptr(bias), ep, ptr(y), ldc, ptr(y16), ld16,
                         ptr(yq), ldyq, ptr(ys), ldys, m, n, k, _stream())
    assert st == 0, st
    torch.cuda.synchronize()
    if y is not None:
        G._assert_sentinel_outside(y, m, n, "y")
    if y16 is not None:
        G._assert_sentinel_outside(y16, m, n, "y_bf16")
    if yq is not None:
        _assert_bytes_outside(yq, m, n, SQ, "yq")
        _assert_bytes_outside(ys, m, n // 32, SS, "ys")
    return y, y16, yq, ys


def _assert_mx_pair_of(y, yq, ys, m, n, what):
    """(yq, ys) is the restated quantiser applied to the f32 values y (all on the device, pitched)."""
    q, s = mx_quantize(y[:m, :n].cpu())
    assert torch.equal(ys[:m, :n // 32].cpu(), s), what + ": scale bytes differ from the quantiser of the stored f32 values"
    assert torch.equal(yq[:m, :n].cpu(), q), what + ": element bytes differ from the quantiser of the stored f32 values"


# =====================================================================================================================
# 1. lane map and packing, exact
# =====================================================================================================================
def _exact_inputs(m, n, k, seed):
    gen = torch.Generator().manual_seed(seed)
    xv, wv = torch.randint(-8, 9, (m, k), generator=gen).float(), torch.randint(-8, 9, (n, k), generator=gen).float()
    xq, wq = xv.to(torch.float8_e4m3fn).view(torch.uint8), wv.to(torch.float8_e4m3fn).view(torch.uint8)
    blk = torch.arange(k // 32)
    xs = (125 + (torch.arange(m)[:, None] + 2 * blk[None, :] + torch.randint(0, 5, (1,), generator=gen)) % 5).to(torch.uint8)
    ws = (125 + (3 * torch.arange(n)[:, None] + blk[None, :] + torch.randint(0, 5, (1,), generator=gen)) % 5).to(torch.uint8)
    xd, wd = mx_dequantize(xq, xs), mx_dequantize(wq, ws)
    assert torch.equal(xd, xv.double() * torch.pow(torch.tensor(2.0, dtype=torch.float64), xs.double() - 127).repeat_interleave(32, dim=1))
    bias = torch.randint(-30, 31, (n,), generator=gen).float()
    res = torch.randint(-50, 51, (m, n), generator=gen).float()
    acc = xd @ wd.t()
    assert float(acc.abs().max()) + 100 < 2.0 ** 20
    return dict(xq=xq, xs=xs, wq=wq, ws=ws, bias=bias, res=res, acc=acc, m=m, n=n, k=k)


def _check_exact(inp, what, epilogues=(EP_BF16, EP_ACCUM, EP_GELU_MX)):
    m, n = inp["m"], inp["n"]
    z = inp["acc"] + inp["bias"].double()
    if EP_BF16 in epilogues:
        _, y16, _, _ = _run(inp, EP_BF16, True)
        assert torch.equal(G._bits(y16[:m, :n]).cpu(), G._bits(z.float().to(BF))), what + ": bf16 epilogue"
        _, y16, _, _ = _run(inp, EP_BF16, False)
        assert torch.equal(G._bits(y16[:m, :n]).cpu(), G._bits(inp["acc"].float().to(BF))), what + ": bf16 epilogue without bias"
    if EP_ACCUM in epilogues:
        y, _, _, _ = _run(inp, EP_ACCUM, True)
        assert torch.equal(y[:m, :n].cpu().double(), z + inp["res"].double()), what + ": accumulating epilogue"
        y, _, _, _ = _run(inp, EP_ACCUM, False)
        assert torch.equal(y[:m, :n].cpu().double(), inp["acc"] + inp["res"].double()), what + ": accumulating epilogue without bias"
    if EP_GELU_MX in epilogues:
        y, _, yq, ys = _run(inp, EP_GELU_MX, True)
        # erf by A&S 7.1.26 (1.5e-7 absolute) and its f32 roundings on a factor in [0, 2], times |z| / 2, and two product roundings
        G._assert_within(y[:m, :n], G._gelu64(z), G.GELU_ABS + 8 * U32 * z.abs(), what, "mx gelu f32 (integer operands)")
        _assert_mx_pair_of(y, yq, ys, m, n, what + ": GELU -> MX epilogue")
        _, _, yq2, ys2 = _run(inp, EP_GELU_MX, True, want_y=False)
        assert torch.equal(yq2, yq) and torch.equal(ys2, ys), what + ": the MX pair without the f32 rows differs"


@gpu
@pytest.mark.parametrize("k", [128, 384])
@pytest.mark.parametrize("n", [32, C - 32, C + 32])
@pytest.mark.parametrize("m", [1, R - 1, R + 1, 2 * R + 37])
def test_lane_map_and_packing_exact(m, n, k):
    _check_exact(_exact_inputs(m, n, k, 17 * m + 3 * n + k), f"exact M={m} N={n} K={k}")


@gpu
def test_tile_walk_exact():
    """6 x 3 = 18 tiles: two XCDs take three tiles, six take two -- both arms of the workgroup -> tile map, every tile once, every epilogue."""
    _check_exact(_exact_inputs(5 * R + 1, 2 * C + 32, 128, 99), "tile walk")


@gpu
@pytest.mark.parametrize("n", [128, 640])
def test_gelu_mx_epilogue_at_the_layernorm_shapes(n):
    """37 rows x 128 and x 640 columns (five column tiles), as the MX LayerNorm: the stored f32 rows inside the GELU bound of the bf16 GEMM, the MX
    pair bit-equal to the quantiser of the STORED f32 values, with and without the f32 rows -- on random operands and on exact ones."""
    m, k = 37, 128
    inp = _random_inputs(m, n, k)
    v, b32, _ = G._nt_reference(inp, True, 1, False)
    y, _, yq, ys = _run(inp, EP_GELU_MX, True)
    G._assert_within(y[:m, :n], v, b32, f"gelu -> mx 37 x {n}", "mx gemm gelu")
    _assert_mx_pair_of(y, yq, ys, m, n, f"gelu -> mx 37 x {n}")
    _, _, yq2, ys2 = _run(inp, EP_GELU_MX, True, want_y=False)
    assert torch.equal(yq2, yq) and torch.equal(ys2, ys)
    _check_exact(_exact_inputs(m, n, k, 5 * n), f"exact gelu -> mx 37 x {n}", epilogues=(EP_GELU_MX,))


@gpu
def test_gemm_refuses_what_it_does_not_take():
    _lib, L = _api()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    y = torch.zeros(1 << 14, dtype=torch.float32, device="cuda")
    p, yp = buf.data_ptr(), y.data_ptr()
    call = lambda n, k, ep=EP_ACCUM, yy=yp: L.ts_mx_gemm_nt(p, k, p, max(k // 32, 4), p, p, None, ep, yy, n, None, 0, None, 0, None, 0, 4, n, k, _stream())
    assert call(32, 128) == 0
    assert call(48, 128) == _lib.TS_EUNSUPPORTED and call(32, 64) == _lib.TS_EUNSUPPORTED and call(32, 160) == _lib.TS_EUNSUPPORTED
    assert call(32, 128, ep=3) == _lib.TS_EINVAL and call(32, 128, yy=None) == _lib.TS_EINVAL and call(32, 128, ep=EP_BF16) == _lib.TS_EINVAL
    assert L.ts_mx_pack_w(p, 128, p, 4, 24, 128, p, p, _stream()) == _lib.TS_EUNSUPPORTED
    assert L.ts_mx_quantize_rows(yp, 0, 48, 4, 48, p, 48, p, 2, _stream()) == _lib.TS_EUNSUPPORTED
    assert L.ts_mx_layernorm_fwd(yp, None, None, yp, yp, 1e-5, 4, 48, None, p, 48, p, 2, _stream()) == _lib.TS_EUNSUPPORTED
    torch.cuda.synchronize()


# =====================================================================================================================
# 2. quantiser
# =====================================================================================================================
@functools.lru_cache(maxsize=None)
def _quantiser_rows():
    """37 rows x 384 columns: the hand-made blocks of the host test first, then random blocks over 24 binades."""
    gen = torch.Generator().manual_seed(3)
    hb = handmade_blocks()
    n_blocks = 37 * 12
    rnd = torch.randn(n_blocks - hb.shape[0], 32, generator=gen) * torch.pow(2.0, torch.randint(-12, 12, (n_blocks - hb.shape[0], 1), generator=gen).float())
    return torch.cat([hb, rnd]).reshape(37, 384)


@gpu
@pytest.mark.parametrize("src_bf16", [0, 1])
def test_quantize_rows_is_bit_equal_to_the_restatement(src_bf16):
    _lib, L = _api()
    rows, k, ld, ldq, lds = 37, 384, 400, 392, 16
    v = _quantiser_rows().to(BF) if src_bf16 else _quantiser_rows()
    q_ref, s_ref = mx_quantize(v)
    src = G._padded(v, ld)                                                    # NaN in the padding
    q, s = _bytes(rows + 2, ldq, SQ), _bytes(rows + 3, lds, SS)
    assert L.ts_mx_quantize_rows(src.data_ptr(), src_bf16, ld, rows, k, q.data_ptr(), ldq, s.data_ptr(), lds, _stream()) == 0
    torch.cuda.synchronize()
    _assert_bytes_outside(q, rows, k, SQ, "q")
    _assert_bytes_outside(s, rows, k // 32, SS, "scales")
    assert torch.equal(s[:rows, :k // 32].cpu(), s_ref), "scale bytes"
    bad = (q[:rows, :k].cpu() != q_ref).nonzero()
    assert bad.numel() == 0, f"element bytes differ at {bad[:5].tolist()}"


# =====================================================================================================================
# 3. MX LayerNorm and the GELU -> MX epilogue
# =====================================================================================================================
@gpu
@pytest.mark.parametrize("c", [128, 640])
def test_mx_layernorm(c):
    _lib, L = _api()
    rows = 37
    gen = torch.Generator().manual_seed(c)
    x = 2.0 * torch.randn(rows, c, generator=gen) + 3.0
    res_h, xb_h = torch.randn(rows, c, generator=gen), torch.randn(c, generator=gen)
    w, b = 1.0 + 0.3 * torch.randn(c, generator=gen), 0.2 * torch.randn(c, generator=gen)
    dx, dres, dxb, dw, db = (z.cuda() for z in (x, res_h, xb_h, w, b))
    ldq, lds = c + 4, c // 32 + 3
    for use_res in (False, True):
        for use_xb in (False, True):
            what = f"mx_layernorm c={c} res={use_res} xbias={use_xb}"
            s64 = x.double() + (res_h.double() if use_res else 0.0) + (xb_h.double() if use_xb else 0.0)
            ref = F.layer_norm(s64, (c,), w.double(), b.double(), eps=1e-5)
            outs = []
            for want_y in (True, False):
                y = torch.full((rows + 2, c), float("nan"), device="cuda") if want_y else None
                q, s = _bytes(rows + 2, ldq, SQ), _bytes(rows + 3, lds, SS)
                st = L.ts_mx_layernorm_fwd(dx.data_ptr(), dres.data_ptr() if use_res else None, dxb.data_ptr() if use_xb else None, dw.data_ptr(),
                                           db.data_ptr(), 1e-5, rows, c, y.data_ptr() if want_y else None, q.data_ptr(), ldq, s.data_ptr(), lds, _stream())
                assert st == 0, st
                torch.cuda.synchronize()
                _assert_bytes_outside(q, rows, c, SQ, what + " q")
                _assert_bytes_outside(s, rows, c // 32, SS, what + " scales")
                outs.append((y, q, s))
            (y, q, s), (_, q2, s2) = outs
            assert bool(torch.isnan(y[rows:]).all()), what + ": rows beyond the last were written"
            err, scale = float((y[:rows].cpu().double() - ref).abs().max()), float(ref.abs().max())
            assert err <= 1e-5 * scale, f"{what}: max error {err:.3e} > 1e-5 x {scale:.3e}"
            _assert_mx_pair_of(y, q, s, rows, c, what)
            assert torch.equal(q2, q) and torch.equal(s2, s), what + ": the MX pair without the f32 rows differs"


# =====================================================================================================================
# 4. the product on random operands, element by element
# =====================================================================================================================
RANDOM_SHAPES = [(m, n, k) for k in (128, 1024) for m in (R + 1, 300) for n in (96, C + 32)]


@functools.lru_cache(maxsize=None)
def _random_inputs(m, n, k):
    """Gaussian rows and weights through the restated quantiser; the float64 product and sum|a b| of the DEQUANTISED values the kernel reads."""
    gen = torch.Generator().manual_seed(7 * m + 5 * n + k)
    xq, xs = mx_quantize(torch.randn(m, k, generator=gen))
    wq, ws = mx_quantize(torch.randn(n, k, generator=gen) / k ** 0.5)
    xd, wd = mx_dequantize(xq, xs), mx_dequantize(wq, ws)
    bias = 0.5 * torch.randn(n, generator=gen)
    res = torch.randn(m, n, generator=gen)
    return dict(xq=xq, xs=xs, wq=wq, ws=ws, xd=xd, wd=wd, bias=bias, res=res, acc=xd @ wd.t(), sabs=C_ACC * (xd.abs() @ wd.abs().t()), m=m, n=n, k=k)


@pytest.mark.parametrize("m,n,k", RANDOM_SHAPES)
def test_bounds_admit_f32_arithmetic_and_are_not_vacuous(m, n, k):
    """torch's own f32 product of the same dequantised operands stays inside every bound.  How far the bound is from vacuous: at K = 128 (one
    instruction, where C_ACC was measured) the median bound of a bf16 result is 1.07 x the bare rounding u16 |y|; at K = 1024 the same factor makes it
    2.7 x (the measured error there is 0.06 of g(k) sum|a b|: the bound form g(k) grows with K, the instruction's error does not)."""
    inp = _random_inputs(m, n, k)
    acc32 = (inp["xd"].float() @ inp["wd"].float().t())
    v, b32, b16 = G._nt_reference(inp, True, 0, False)
    assert bool((((acc32 + inp["bias"]).double() - v).abs() <= b32).all())
    assert float((b16 / (G.U16 * v.abs())).median()) < (1.5 if k == 128 else 3.0)
    v, b32, _ = G._nt_reference(inp, True, 0, True)
    assert bool((((acc32 + inp["bias"]) + inp["res"]).double().sub(v).abs() <= b32).all())
    v, b32, _ = G._nt_reference(inp, True, 1, False)
    assert bool((F.gelu(acc32 + inp["bias"]).double().sub(v).abs() <= b32).all())


@gpu
@pytest.mark.parametrize("m,n,k", RANDOM_SHAPES)
def test_gemm_random_operands_element_by_element(m, n, k):
    """C_ACC = 4; the worst measured error / (g(k) sum|a b|) is 2.80 at K = 128 (one instruction) and 0.062 at K = 1024: module docstring."""
    inp = _random_inputs(m, n, k)
    what = f"mx gemm M={m} N={n} K={k}"
    v, _, b16 = G._nt_reference(inp, True, 0, False)
    _, y16, _, _ = _run(inp, EP_BF16, True)
    G._assert_within(y16[:m, :n], v, b16, what + " bias -> bf16", "mx gemm bf16")
    v, b32, _ = G._nt_reference(inp, True, 0, True)
    y, _, _, _ = _run(inp, EP_ACCUM, True)
    G._assert_within(y[:m, :n], v, b32, what + " bias, in place", "mx gemm accumulate")
    v, b32, _ = G._nt_reference(inp, False, 0, True)
    y, _, _, _ = _run(inp, EP_ACCUM, False)
    G._assert_within(y[:m, :n], v, b32, what + " in place", "mx gemm accumulate")
    v, b32, _ = G._nt_reference(inp, True, 1, False)
    y, _, yq, ys = _run(inp, EP_GELU_MX, True)
    G._assert_within(y[:m, :n], v, b32, what + " bias, GELU", "mx gemm gelu")
    _assert_mx_pair_of(y, yq, ys, m, n, what + " GELU -> MX")
