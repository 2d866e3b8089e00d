"""Both matrix-core GEMMs -- csrc/gemm_nt.hip (bf16, token-major, fused epilogue) and csrc/gemm_f32.hip (f32 matrix-core instruction) -- through the
C ABI against a float64 product of the very operand values the kernel reads, ELEMENT BY ELEMENT, every row asserting through
ts_gemm_nt_launch_config / ts_gemm_f32_launch_config which instantiation and which fetch path it ran.

Conventions of every row:
  * output buffers have a pitch larger than n (ldc, ld16 and ld_res all different) and extra rows behind M, pre-filled with a sentinel bit pattern
    (a NaN); after the call everything outside [0, M) x [0, n) is still the sentinel, bit for bit;
  * operand padding (columns [k, lda) and [k, ldw); in gemm_f32 the pitch padding of both layouts and the gaps between batches and outer
    contraction steps) holds NaN: every stored output must be finite and inside its bound;
  * the tile-walk rows use integer operands (|x|, |w| <= 4, K = 32, integer bias): every f32 sum is exact, the comparison is torch.equal.

Bounds per element, u32 = 2^-24, u16 = 2^-8, g(n) = n u32 / (1 - n u32) (profiles/gemm_kernel_checks.md derives them):
  gemm_f32   E = g(nkb K) sum|a b|  (+ u32 (|acc| + |bias|))  (+ u32 (|acc + bias| + |c_old|) with beta);  bf16 result: u16 (|v| + E) + E
  gemm_nt    E = g(K) sum|x w|  (+ u32 (|acc| + |bias|));  GELU: 1.13 E + 2e-6 (|z| <= 8, the erf term of tests/test_gpu_w2v_kernels.py; 1.13 >
             sup |gelu'|);  SiLU: 1.1 E + (|z| + 7) u32 |silu(z)| (1.1 > sup |silu'|; __expf, 1 + e, reciprocal, product);
             residual: + u32 (|a| + |res|);  bf16 result: u16 (|v| + E) + E
test_bounds_admit_f32_arithmetic_and_are_not_vacuous (no GPU) shows for every row that torch's own float32 CPU product stays inside the bound and
that the median bound of a bf16 result is below 1.5 x the bare rounding term u16 |y|.
"""
import ctypes as C
import functools
import math
import zlib
from dataclasses import dataclass

import pytest
import torch

gpu = pytest.mark.gpu

U32, U16 = 2.0 ** -24, 2.0 ** -8
BF = torch.bfloat16
NAN = float("nan")
S32, S16 = 0x7FA5A5A5, 0x7FA5                     # sentinels: NaN bit patterns no kernel produces
LIP_GELU, LIP_SILU, GELU_ABS = 1.13, 1.1, 2e-6


def g(n):
    return n * U32 / (1.0 - n * U32)


def _api():
    from thunder_speech_amd import _lib
    return _lib, _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _gelu64(z):
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def _silu64(z):
    return z * torch.sigmoid(z)


def _sentinel(rows, pitch, dtype):
    if dtype == torch.float32:
        return torch.full((rows, pitch), S32, dtype=torch.int32, device="cuda").view(torch.float32)
    return torch.full((rows, pitch), S16, dtype=torch.int16, device="cuda").view(BF)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def _assert_sentinel_outside(buf, m, n, what):
    v, s = _bits(buf), (S32 if buf.dtype == torch.float32 else S16)
    assert bool((v[m:] == s).all()), f"{what}: rows at and beyond M were written"
    assert bool((v[:m, n:] == s).all()), f"{what}: columns in [n, pitch) were written"


WORST = {}


def _assert_within(got, ref, bound, what, kind):
    """|got - ref| <= bound for every element; got on the device, ref / bound float64 on the host.  Prints the worst error / bound."""
    got = got.detach().double().cpu()
    assert bool(torch.isfinite(got).all()), f"{what}: a stored output is not finite (unwritten, or padding reached it)"
    ratio = ((got - ref).abs() / bound)
    worst = float(ratio.max())
    WORST[kind] = max(WORST.get(kind, 0.0), worst)
    print(f"[gemm-check] {what} {kind}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0, f"{what} {kind}: {int((ratio > 1).sum())} elements outside their bound, worst error / bound {worst:.3f} at " \
                         f"{tuple(int(i) for i in (ratio == ratio.max()).nonzero()[0])}"


# =====================================================================================================================
# gemm_nt
# =====================================================================================================================
NT_NAMES = ("n_mt", "n_nt", "blk_c", "grid_x", "grid_y", "threads", "lds_bytes", "instantiation", "epilogue")
NT_LDS, NT_LDS_SILU, NT_PACKED, NT_PACKED_SILU = 0, 1, 2, 3
EP_BF16, EP_F32 = 0, 1


def _nt_query(L, x, lda, w, ldw, wf, res, ld_res, y, ldc, y16, ld16, rows, n, k, act, batch=1):
    out = [C.c_int32(-7) for _ in NT_NAMES]
    st = L.ts_gemm_nt_launch_config(x, lda, w, ldw, wf, res, ld_res, y, ldc, y16, ld16, rows, n, k, act, batch, *[C.byref(o) for o in out])
    return st, dict(zip(NT_NAMES, (o.value for o in out)))


@functools.lru_cache(maxsize=None)
def _nt_inputs(m, n, k, seed):
    """bf16 operands, f32 bias and residual on the host, the float64 product of the bf16 values and sum|x w|."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(m, k, generator=gen).to(BF)
    w = (torch.randn(n, k, generator=gen) / k ** 0.5).to(BF)
    bias = 0.5 * torch.randn(n, generator=gen)
    res = torch.randn(m, n, generator=gen)
    acc = x.double() @ w.double().t()
    sabs = x.double().abs() @ w.double().abs().t()
    return dict(x=x, w=w, bias=bias, res=res, acc=acc, sabs=sabs, m=m, n=n, k=k)


def _nt_exact_inputs(m, n, k, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(-4, 5, (m, k), generator=gen).to(BF)
    w = torch.randint(-4, 5, (n, k), generator=gen).to(BF)
    bias = torch.randint(-30, 31, (n,), generator=gen).float()
    acc = x.double() @ w.double().t()
    return dict(x=x, w=w, bias=bias, res=None, acc=acc, sabs=None, m=m, n=n, k=k)


def _nt_reference(inp, use_bias, act, use_res):
    """(v, bound of the f32 result, bound of the bf16 result), float64 on the host."""
    acc, k = inp["acc"], inp["k"]
    e = g(k) * inp["sabs"]
    z = acc
    if use_bias:
        b = inp["bias"].double()
        e = e + U32 * (acc.abs() + b.abs())
        z = acc + b
    if act:
        assert float(z.abs().max()) <= 8.0                                   # the range the activation terms are stated for
    if act == 1:
        a, e = _gelu64(z), LIP_GELU * e + GELU_ABS
    elif act == 2:
        a = _silu64(z)
        e = LIP_SILU * e + (z.abs() + 7.0) * U32 * a.abs()
    else:
        a = z
    v = a
    if use_res:
        r = inp["res"].double()
        e = e + U32 * (a.abs() + r.abs())
        v = a + r
    return v, e, U16 * (v.abs() + e) + e


def _padded(t, pitch, rows=None):
    """t [r][c] on the device as rows of `pitch` elements, the padding NaN."""
    out = torch.full((rows or t.shape[0], pitch), NAN, dtype=t.dtype, device="cuda")
    out[:t.shape[0], :t.shape[1]] = t.cuda()
    return out


def _pack_w(L, w_dev, ldw, n, k):
    wf = torch.full((n * k,), NAN, dtype=BF, device="cuda")
    assert L.ts_gemm_nt_pack_w(w_dev.data_ptr(), ldw, n, k, wf.data_ptr(), _stream()) == 0
    return wf


def _run_nt(inp, family, use_bias, act, res_mode, form):
    """One product.  family "lds" | "packed"; res_mode None | "res" | "inplace"; form "f32" | "bf16" | "both".  act 2 (SiLU) goes through
    ts_conformer_linear_fwd, whose weights are dense (ldw = k).  Asserts the query, returns the whole (pitched) output buffers."""
    _lib, L = _api()
    m, n, k = inp["m"], inp["n"], inp["k"]
    lda, ldw = k + 8, (k if act == 2 else k + 16)
    ldc, ld16 = n + 12, n + 24
    ld_res = ldc if res_mode == "inplace" else n + 20
    x, w = _padded(inp["x"], lda), _padded(inp["w"], ldw)
    wf = _pack_w(L, w, ldw, n, k) if family == "packed" else None
    bias = inp["bias"].cuda() if use_bias else None
    y = _sentinel(m + 3, ldc, torch.float32) if form in ("f32", "both") else None
    y16 = _sentinel(m + 5, ld16, BF) if form in ("bf16", "both") else None
    res = None
    if res_mode == "inplace":
        assert y is not None
        y[:m, :n] = inp["res"].cuda()
        res = y
    elif res_mode == "res":
        res = _sentinel(m + 1, ld_res, torch.float32)
        res[:m, :n] = inp["res"].cuda()
    ptr = lambda t: None if t is None else t.data_ptr()
    st, q = _nt_query(L, x.data_ptr(), lda, w.data_ptr(), ldw, ptr(wf), ptr(res), ld_res if res is not None else 0, ptr(y), ldc if y is not None else 0,
                      ptr(y16), ld16 if y16 is not None else 0, m, n, k, act)
    assert st == 0, st
    tile = 128 if family == "packed" else 256
    want = dict(n_mt=(m + tile - 1) // tile, n_nt=(n + 255) // 256, grid_y=1, threads=256 if family == "packed" else 512,
                lds_bytes=4 * 128 * 144 if family == "packed" else 8 * 128 * 144,
                instantiation=(NT_PACKED if family == "packed" else NT_LDS) + (1 if act == 2 else 0),
                epilogue=EP_BF16 if (form == "bf16" and res is None) else EP_F32)
    want["grid_x"] = want["n_mt"] * want["n_nt"]
    assert {key: q[key] for key in want} == want, (q, want)
    if act == 2:
        st = L.ts_conformer_linear_fwd(x.data_ptr(), lda, w.data_ptr(), ptr(wf), ptr(bias), ptr(res), ld_res if res is not None else 0, ptr(y),
                                       ldc if y is not None else 0, ptr(y16), ld16 if y16 is not None else 0, m, n, k, 2, 1, _stream())
    elif family == "packed":
        st = L.ts_gemm_nt_bf16_packed(x.data_ptr(), lda, w.data_ptr(), ldw, wf.data_ptr(), ptr(bias), ptr(res), ld_res if res is not None else 0, ptr(y),
                                      ldc if y is not None else 0, ptr(y16), ld16 if y16 is not None else 0, m, n, k, act, _stream())
    else:
        st = L.ts_gemm_nt_bf16(x.data_ptr(), lda, w.data_ptr(), ldw, ptr(bias), ptr(res), ld_res if res is not None else 0, ptr(y),
                               ldc if y is not None else 0, ptr(y16), ld16 if y16 is not None else 0, m, n, k, act, _stream())
    assert st == 0, st
    torch.cuda.synchronize()
    if res_mode == "res":                                                   # the residual is read only
        assert torch.equal(res[:m, :n], inp["res"].cuda())
        _assert_sentinel_outside(res, m, n, "residual")
    return y, y16, q


def _check_nt(inp, family, use_bias, act, res_mode, form, what):
    y, y16, q = _run_nt(inp, family, use_bias, act, res_mode, form)
    m, n = inp["m"], inp["n"]
    v, b32, b16 = _nt_reference(inp, use_bias, act, res_mode is not None)
    what = f"{what} {family} bias={int(use_bias)} act={act} res={res_mode} form={form}"
    if y is not None:
        _assert_sentinel_outside(y, m, n, what + " y")
        _assert_within(y[:m, :n], v, b32, what, "gemm_nt f32")
    if y16 is not None:
        _assert_sentinel_outside(y16, m, n, what + " y_bf16")
        _assert_within(y16[:m, :n], v, b16, what, "gemm_nt bf16")
    if y is not None and y16 is not None:                                   # the bf16 result is the rounding of the f32 value after the residual
        assert torch.equal(_bits(y16[:m, :n]), _bits(y[:m, :n].to(BF))), what + ": y_bf16 is not the rounding of y"
    return q


NT_FAMILIES = [("lds", 0), ("packed", 0), ("lds", 2), ("packed", 2)]        # (family, act): the four instantiations
PIPELINE_KS = [1, 2, 3, 4, 5, 6, 9]                                         # K / 32: every arm of the prologue and tail waits, both loop parities
ROW_EDGE_M = [1, 15, 127, 128, 129, 255, 256, 257]


@gpu
@pytest.mark.parametrize("family,act", NT_FAMILIES)
@pytest.mark.parametrize("ks", PIPELINE_KS)
def test_nt_pipeline_depth(ks, family, act):
    """K / 32 half-stages, M = 257 (a full tile and one row), N = 64: prologue and tail of the ring for every remaining depth."""
    inp = _nt_inputs(257, 64, 32 * ks, 1000 + ks)
    _check_nt(inp, family, True, act, None, "both", f"pipeline K/32={ks}")
    _check_nt(inp, family, True, act, None, "bf16", f"pipeline K/32={ks}")


@gpu
@pytest.mark.parametrize("family", ["lds", "packed"])
@pytest.mark.parametrize("n", [32, 96])
@pytest.mark.parametrize("m", ROW_EDGE_M)
def test_nt_row_edges(m, n, family):
    """Rows at and next to the 128- and 256-row tiles; N = 32 leaves three wave columns entirely beyond N, N = 96 a partial one."""
    inp = _nt_inputs(m, n, 64, 2000 + 10 * m + n)
    _check_nt(inp, family, True, 0, None, "both", f"rows M={m} N={n}")
    _check_nt(inp, family, True, 0, None, "bf16", f"rows M={m} N={n}")


@gpu
@pytest.mark.parametrize("family", ["lds", "packed"])
@pytest.mark.parametrize("act", [0, 1, 2])
def test_nt_epilogue_forms(act, family):
    """{f32, bf16, both} x {bias, none} x {no residual, residual, residual in place} x activation; the bf16-only form takes no residual."""
    inp = _nt_inputs(300, 96, 64, 3000)
    for form in ("f32", "bf16", "both"):
        for use_bias in (True, False):
            for res_mode in ((None,) if form == "bf16" else (None, "res", "inplace")):
                _check_nt(inp, family, use_bias, act, res_mode, form, "epilogue")


# (n_mt, n_nt, blk_c): short last band, every block width, fewer tiles than XCDs, tile counts that are no multiple of 8.  A short band is walked
# differently from a full one only where it holds more than one block (n_nt > blk_c): (13, 9), (35, 5), (3, 7), (1, 5) and, for blk_c 4, (11, 8)
WALK = [(11, 4, 4), (13, 3, 3), (13, 9, 3), (19, 2, 2), (35, 5, 1), (3, 7, 1), (1, 5, 1), (2, 4, 4), (11, 8, 4)]


@gpu
@pytest.mark.parametrize("family", ["lds", "packed"])
@pytest.mark.parametrize("n_mt,n_nt,blk_c", WALK)
def test_nt_tile_walk_is_exact(n_mt, n_nt, blk_c, family):
    """Integer operands, K = 32, a column bias: every element of every tile equals the float64 product (torch.equal), so a skipped, doubled or
    misplaced tile cannot pass; the last row tile is ragged (37 rows)."""
    _lib, L = _api()
    tile = 128 if family == "packed" else 256
    m, n, k = (n_mt - 1) * tile + 37, 256 * n_nt, 32
    inp = _nt_exact_inputs(m, n, k, 4000 + 100 * n_mt + n_nt)
    ref = (inp["acc"] + inp["bias"].double()).cuda()
    for form in ("both", "bf16"):
        y, y16, q = _run_nt(inp, family, True, 0, None, form)
        assert (q["n_mt"], q["n_nt"], q["blk_c"], q["grid_x"]) == (n_mt, n_nt, blk_c, n_mt * n_nt), q
        if y is not None:
            _assert_sentinel_outside(y, m, n, "walk y")
            assert torch.equal(y[:m, :n].double(), ref), f"walk ({n_mt}, {n_nt}) {family} {form}: f32 result differs from the exact product"
        _assert_sentinel_outside(y16, m, n, "walk y_bf16")
        assert torch.equal(y16[:m, :n], ref.to(BF)), f"walk ({n_mt}, {n_nt}) {family} {form}: bf16 result differs from the rounded exact product"


CONV = [(3, 2), (2, 2)]                                                     # (kernel, stride)
CONV_B, CONV_T, CONV_CI, CONV_CO = 3, 601, 32, 64


@functools.lru_cache(maxsize=None)
def _conv_inputs(kernel, stride):
    gen = torch.Generator().manual_seed(5000 + kernel)
    t_out = (CONV_T - kernel) // stride + 1
    x = torch.randn(CONV_B, CONV_T, CONV_CI, generator=gen).to(BF)
    w = (torch.randn(CONV_CO, kernel * CONV_CI, generator=gen) / (kernel * CONV_CI) ** 0.5).to(BF)
    bias = 0.5 * torch.randn(CONV_CO, generator=gen)
    cols = torch.stack([x[:, stride * t: stride * t + kernel].reshape(CONV_B, -1) for t in range(t_out)], 1).reshape(CONV_B * t_out, -1)   # im2col
    acc = cols.double() @ w.double().t()
    sabs = cols.double().abs() @ w.double().abs().t()
    return dict(x=x, x2d=cols, w=w, bias=bias, res=None, acc=acc, sabs=sabs, m=CONV_B * t_out, n=CONV_CO, k=kernel * CONV_CI, t_out=t_out)


@gpu
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("kernel,stride", CONV)
def test_nt_overlapping_rows_and_batch_through_the_conv_layer(kernel, stride, packed):
    """ts_w2v_conv_fwd in bf16 mode: rows of pitch stride * c_in under K = kernel * c_in, three clips on grid.y with their own sx / sy."""
    _lib, L = _api()
    inp = _conv_inputs(kernel, stride)
    t_out, k, n, rows = inp["t_out"], inp["k"], CONV_CO, inp["m"]
    x, w, bias = inp["x"].cuda(), inp["w"].cuda(), inp["bias"].cuda()
    wf = _pack_w(L, w, k, n, k) if packed else None
    for act in (0, 1):
        v, b32, b16 = _nt_reference(inp, True, act, False)
        for want16 in (False, True):
            y, y16 = _sentinel(rows + 4, n, torch.float32), _sentinel(rows + 4, n, BF)
            st, q = _nt_query(L, x.data_ptr(), stride * CONV_CI, w.data_ptr(), k, wf.data_ptr() if packed else None, None, 0,
                              None if want16 else y.data_ptr(), n, y16.data_ptr() if want16 else None, n, t_out, n, k, act, CONV_B)
            assert st == 0 and q["grid_y"] == CONV_B and q["instantiation"] == (NT_PACKED if packed else NT_LDS), (st, q)
            assert q["epilogue"] == (EP_BF16 if want16 else EP_F32) and q["n_mt"] == (t_out + (127 if packed else 255)) // (128 if packed else 256)
            st = L.ts_w2v_conv_fwd(x.data_ptr(), CONV_B, CONV_T, CONV_CI, w.data_ptr(), bias.data_ptr(), n, kernel, stride, act, 1, y.data_ptr(),
                                   y16.data_ptr() if want16 else None, wf.data_ptr() if packed else None, _stream())
            assert st == 0, st
            torch.cuda.synchronize()
            what = f"conv kernel={kernel} stride={stride} packed={packed} act={act} bf16={want16}"
            out, other = (y16, y) if want16 else (y, y16)
            _assert_sentinel_outside(out, rows, n, what)
            _assert_sentinel_outside(other, 0, n, what + " (the output not asked for)")
            _assert_within(out[:rows], v, b16 if want16 else b32, what, "gemm_nt bf16" if want16 else "gemm_nt f32")


SPLITK = [(300, 96, 256, 1), (300, 96, 256, 2), (129, 64, 288, 3), (257, 256, 2048, 8)]


@functools.lru_cache(maxsize=None)
def _splitk_inputs(rows, n, k, splits):
    gen = torch.Generator().manual_seed(6000 + k + splits)
    x, w = torch.randn(rows, k, generator=gen).to(BF), (torch.randn(n, k, generator=gen) / k ** 0.5).to(BF)
    ks = k // splits
    xs, ws = x.double().view(rows, splits, ks).transpose(0, 1), w.double().view(n, splits, ks).transpose(0, 1)
    return dict(x=x, w=w, parts=xs @ ws.transpose(1, 2), sabs=xs.abs() @ ws.abs().transpose(1, 2))


def _splitk_bounds(inp, k, splits):
    """Bounds of each part and of their ordered f32 sum: splits - 1 additions, each rounding a partial sum of the parts."""
    e_parts = g(k // splits) * inp["sabs"]
    mag = inp["parts"].abs() + e_parts
    return e_parts, e_parts.sum(0) + g(max(splits - 1, 0)) * mag.sum(0) if splits > 1 else e_parts[0]


@gpu
@pytest.mark.parametrize("rows,n,k,splits", SPLITK)
def test_nt_split_k_parts_and_their_ordered_sum(rows, n, k, splits):
    _lib, L = _api()
    inp = _splitk_inputs(rows, n, k, splits)
    lda, ldw, ks = k + 8, k + 24, k // splits
    x, w = _padded(inp["x"], lda), _padded(inp["w"], ldw)
    parts = _sentinel(splits * rows + 2, n, torch.float32)
    st, q = _nt_query(L, x.data_ptr(), lda, w.data_ptr(), ldw, None, None, 0, parts.data_ptr(), n, None, 0, rows, n, ks, 0, splits)
    assert st == 0 and (q["grid_y"], q["instantiation"], q["epilogue"], q["n_mt"], q["n_nt"]) == (splits, NT_LDS, EP_F32, (rows + 255) // 256, (n + 255) // 256)
    assert L.ts_gemm_nt_bf16_splitk(x.data_ptr(), lda, w.data_ptr(), ldw, parts.data_ptr(), rows, n, k, splits, _stream()) == 0
    out = _sentinel(rows + 2, n, torch.float32)
    assert L.ts_w2v_sum_parts(parts.data_ptr(), out.data_ptr(), rows * n, splits, _stream()) == 0
    torch.cuda.synchronize()
    what = f"split-K rows={rows} n={n} k={k} splits={splits}"
    _assert_sentinel_outside(parts, splits * rows, n, what + " parts")
    _assert_sentinel_outside(out, rows, n, what + " sum")
    e_parts, e_sum = _splitk_bounds(inp, k, splits)
    got = parts[:splits * rows].view(splits, rows, n)
    for z in range(splits):
        _assert_within(got[z], inp["parts"][z], e_parts[z], f"{what} part {z}", "gemm_nt f32")
    ordered = got[0].clone()
    for z in range(1, splits):
        ordered = ordered + got[z]
    assert torch.equal(_bits(out[:rows]), _bits(ordered)), what + ": ts_w2v_sum_parts is not the ordered f32 sum of the parts"
    _assert_within(out[:rows], inp["parts"].sum(0), e_sum, what + " sum", "split-K sum")


def test_nt_refusals_through_the_query():
    """Every refusal of the launcher, asked of the query alone: nothing is launched, no device is needed."""
    _lib, L = _api()
    E, U = _lib.TS_EINVAL, _lib.TS_EUNSUPPORTED
    base = dict(x=1 << 20, lda=72, w=2 << 20, ldw=80, wf=3 << 20, res=4 << 20, ld_res=116, y=5 << 20, ldc=108, y16=6 << 20, ld16=120, rows=300, n=96, k=64,
                act=0, batch=1)
    order = ("x", "lda", "w", "ldw", "wf", "res", "ld_res", "y", "ldc", "y16", "ld16", "rows", "n", "k", "act", "batch")

    def ask(**kw):
        a = {**base, **kw}
        return _nt_query(L, *[a[name] for name in order])

    st, q = ask()
    assert st == 0 and q == dict(n_mt=3, n_nt=1, blk_c=1, grid_x=3, grid_y=1, threads=256, lds_bytes=73728, instantiation=NT_PACKED, epilogue=EP_F32), (st, q)
    st, q = ask(wf=None, act=2, y=None, ldc=0, res=None, ld_res=0, rows=257, n=2304, ld16=2328)
    assert st == 0 and q == dict(n_mt=2, n_nt=9, blk_c=3, grid_x=18, grid_y=1, threads=512, lds_bytes=147456, instantiation=NT_LDS_SILU, epilogue=EP_BF16)
    for kw in (dict(n=100, ldc=112, ld16=112, ld_res=116), dict(k=48), dict(lda=76), dict(ldw=84), dict(ldc=110), dict(ld16=124), dict(ld_res=118)):
        st, q = ask(**kw)
        assert st == U and set(q.values()) == {-7}, (kw, st, q)                              # and a refusal writes nothing
    assert ask(ldw=56)[0] == E                                                              # ldw < k, as ts_gemm_nt_bf16 answers it
    for name in ("x", "w", "y", "y16", "res", "wf"):
        for off in (2, 8):
            assert ask(**{name: base[name] + off})[0] == U, (name, off)
    # 31-bit byte offsets of the last row of either operand
    lim = (1 << 30) - 1                                                                     # ((rows - 1) lda + k) * 2 >= 2^31 - 1 is refused
    rows = (lim - 64) // 72 + 1
    assert ask(rows=rows)[0] == 0 and ask(rows=rows + 1)[0] == U
    n_ok = ((lim - 64) // 80 + 1) // 32 * 32
    big = dict(n=n_ok, ldc=n_ok + 12, ld16=n_ok + 24, ld_res=n_ok + 20)
    assert ask(**big)[0] == 0
    n_bad = n_ok + 32
    assert ask(n=n_bad, ldc=n_bad + 12, ld16=n_bad + 24, ld_res=n_bad + 20)[0] == U
    for kw in (dict(act=-1), dict(act=3), dict(x=None), dict(w=None), dict(y=None, y16=None), dict(rows=0), dict(n=0), dict(k=0), dict(batch=0), dict(lda=-8),
               dict(ldc=88), dict(ld16=88), dict(ld_res=92)):
        assert ask(**kw)[0] == E, kw
    out = [C.c_int32() for _ in NT_NAMES]
    for hole in range(len(out)):
        refs = [None if i == hole else C.byref(o) for i, o in enumerate(out)]
        assert L.ts_gemm_nt_launch_config(*[base[name] for name in order], *refs) == E


# =====================================================================================================================
# gemm_f32
# =====================================================================================================================
F32_NAMES = ("a_kc", "b_kc", "vec_a", "vec_b", "grid_x", "grid_z", "stages")


def _r4(n):
    return (n + 3) // 4 * 4


@dataclass(frozen=True)
class F32Case:
    name: str
    m: int
    n: int
    k: int
    a_kc: bool
    b_kc: bool
    bf: bool = False                  # bf16 operands
    out_bf: bool = False
    nkb: int = 1
    batch: int = 1
    batch2: int = 1
    beta: bool = False
    bias: bool = False
    a_pad: int = 4                    # pitch = round_up(contiguous extent, 4) + pad: an odd pad is an odd pitch
    b_pad: int = 8
    a_off: int = 0                    # base offset in elements (f32: 1 = 4 bytes; bf16: 2 = 4 bytes)
    b_off: int = 0
    sk_odd: bool = False              # odd strides of the outer contraction loop
    sa_zero: bool = False             # A shared by the first batch level
    sb2_zero: bool = False            # B shared by the second batch level
    b2: bool = False                  # through ts_gemm_f32_b2
    vec: tuple = (1, 1)               # the fetch paths this row is written to take


def _layout_table():
    """All four layouts x f32 / bf16 operands: a full-stage row on the vector path, a K-tail row, and a row on the element path (odd pitch or a base
    off by 4 bytes) for each of the eight instantiations, M, N in {1, 31, 33, 127, 128, 129}, K in {1, 2, 15, 16, 17, 33}."""
    full = [(128, 128, 16), (129, 33, 16), (33, 129, 16), (127, 31, 16), (31, 127, 16), (1, 128, 16), (128, 1, 16), (129, 129, 16)]
    tail = [(33, 127, 17), (127, 129, 33), (129, 31, 15), (31, 33, 2), (1, 1, 1), (128, 33, 33), (129, 127, 17), (33, 128, 15)]
    elem = [(127, 33, 33), (33, 31, 17), (129, 128, 1), (31, 129, 2), (128, 127, 15), (1, 33, 16), (33, 1, 33), (129, 129, 17)]
    rows, i = [], 0
    for bf in (False, True):
        for a_kc in (True, False):
            for b_kc in (True, False):
                tag = f"{'bf16' if bf else 'f32'} a_kc={int(a_kc)} b_kc={int(b_kc)}"
                rows.append(F32Case(f"{tag} full stage", *full[i], a_kc, b_kc, bf=bf))
                rows.append(F32Case(f"{tag} K tail", *tail[i], a_kc, b_kc, bf=bf))
                # element path: alternately an odd pitch of A with a base of B off by 4 bytes, and the reverse; every third row only one operand
                kind = i % 3
                off = 2 if bf else 1
                if kind == 0:
                    rows.append(F32Case(f"{tag} odd pitch A, base B + 4 bytes", *elem[i], a_kc, b_kc, bf=bf, a_pad=1, b_off=off, vec=(0, 0)))
                elif kind == 1:
                    rows.append(F32Case(f"{tag} base A + 4 bytes, odd pitch B", *elem[i], a_kc, b_kc, bf=bf, a_off=off, b_pad=3, vec=(0, 0)))
                else:
                    rows.append(F32Case(f"{tag} odd pitch A only", *elem[i], a_kc, b_kc, bf=bf, a_pad=3, vec=(0, 1)))
                    rows.append(F32Case(f"{tag} base B + 4 bytes only", *elem[i], a_kc, b_kc, bf=bf, b_off=off, vec=(1, 0)))
                i += 1
    return rows


F32_LAYOUTS = _layout_table()
F32_OUTER = [F32Case(f"outer loop a_kc={int(a)} b_kc={int(b)} {'odd' if odd else 'aligned'} ska/skb", 70, 36, 20, a, b, nkb=3, sk_odd=odd, vec=(0, 0) if odd else (1, 1))
             for a, b in ((True, False), (False, True), (True, True)) for odd in (False, True)]
F32_BATCH2 = [F32Case("two batch levels", 70, 36, 24, True, False, batch=2, batch2=3, b2=True, bias=True),
              F32Case("two batch levels, beta, outer loop", 33, 129, 20, False, True, batch=2, batch2=3, nkb=2, beta=True, b2=True),
              F32Case("two batch levels, A shared by the first", 70, 36, 24, True, True, batch=2, batch2=3, beta=True, sa_zero=True, b2=True),
              F32Case("two batch levels, B shared by the second", 70, 36, 24, False, False, batch=2, batch2=3, beta=True, bias=True, sb2_zero=True, b2=True)]
F32_EPILOGUE = [F32Case(f"epilogue bf16_in={int(bf)} bias={int(bias)} beta={int(beta)} bf16_out={int(ob)}", 70, 36, 24, True, False, bf=bf, bias=bias, beta=beta,
                        out_bf=ob) for bf in (False, True) for bias in (False, True) for beta in (False, True) for ob in (False, True)]
F32_ALL = F32_LAYOUTS + F32_OUTER + F32_BATCH2 + F32_EPILOGUE


def _f32_geometry(c):
    """Strides (elements) of a case: (a_rs, a_cs, sa, sa2, ska, size of A), the same for B, (ldc, sc, sc2, size of C)."""
    def operand(contig, outer, pad, off, zero1, zero2):
        ld = _r4(contig) + pad
        sk = outer * ld + 8 + (1 if c.sk_odd else 0)
        s2 = 0 if (zero2 or c.batch2 == 1) else c.nkb * sk + 12                 # ts_gemm_f32 has no second level: its stride is 0
        s1 = 0 if zero1 else c.batch2 * (c.nkb * sk + 12) + 20
        size = off + (c.batch - 1) * s1 + (c.batch2 - 1) * s2 + (c.nkb - 1) * sk + outer * ld + 8
        return ld, s1, s2, sk, size
    a_ld, sa, sa2, ska, a_size = operand(c.k if c.a_kc else c.m, c.m if c.a_kc else c.k, c.a_pad, c.a_off, c.sa_zero, False)
    b_ld, sb, sb2, skb, b_size = operand(c.k if c.b_kc else c.n, c.n if c.b_kc else c.k, c.b_pad, c.b_off, False, c.sb2_zero)
    a = (a_ld, 1, sa, sa2, ska, a_size) if c.a_kc else (1, a_ld, sa, sa2, ska, a_size)
    b = (1, b_ld, sb, sb2, skb, b_size) if c.b_kc else (b_ld, 1, sb, sb2, skb, b_size)
    ldc = c.n + 5
    sc2 = (c.m + 2) * ldc + 3
    sc = c.batch2 * sc2 + 7
    return a, b, (ldc, sc, sc2, (c.batch - 1) * sc + (c.batch2 - 1) * sc2 + (c.m + 2) * ldc + 9)


def _index(shape, strides, off):
    idx = torch.full((1,) * len(shape), off, dtype=torch.int64)
    for d, (n, s) in enumerate(zip(shape, strides)):
        view = [1] * len(shape)
        view[d] = n
        idx = idx + (torch.arange(n, dtype=torch.int64) * s).view(view)
    return idx.reshape(-1)


@functools.lru_cache(maxsize=None)
def _f32_inputs(c):
    """Logical operands [batch][batch2][nkb][m][k] / [..][k][n] (shared along a zero stride), c_old, bias, the float64 product and sum|a b|."""
    gen = torch.Generator().manual_seed(zlib.crc32(c.name.encode()))
    dt = BF if c.bf else torch.float32
    a = torch.randn(1 if c.sa_zero else c.batch, c.batch2, c.nkb, c.m, c.k, generator=gen).to(dt).expand(c.batch, -1, -1, -1, -1)
    b = torch.randn(c.batch, 1 if c.sb2_zero else c.batch2, c.nkb, c.k, c.n, generator=gen).to(dt).expand(-1, c.batch2, -1, -1, -1)
    c_old = torch.randn(c.batch, c.batch2, c.m, c.n, generator=gen).to(BF if c.out_bf else torch.float32)
    bias = torch.randn(c.n, generator=gen)
    acc = torch.einsum("xyjmk,xyjkn->xymn", a.double(), b.double())
    sabs = torch.einsum("xyjmk,xyjkn->xymn", a.double().abs(), b.double().abs())
    return dict(a=a, b=b, c_old=c_old, bias=bias, acc=acc, sabs=sabs)


def _f32_reference(c, inp):
    acc = inp["acc"]
    e = g(c.nkb * c.k) * inp["sabs"]
    v = acc
    if c.bias:
        bv = inp["bias"].double()
        e = e + U32 * (acc.abs() + bv.abs())
        v = acc + bv
    if c.beta:
        old = inp["c_old"].double()                                          # with a bf16 result: the bf16 value the kernel reads
        e = e + U32 * (v.abs() + old.abs())
        v = v + old
    return v, (U16 * (v.abs() + e) + e if c.out_bf else e)


def _f32_query(L, c, a_ptr, b_ptr, c_ptr, ga, gb, gc):
    out = [C.c_int32(-7) for _ in F32_NAMES]
    st = L.ts_gemm_f32_launch_config(a_ptr, ga[0], ga[1], ga[2], ga[3], ga[4], b_ptr, gb[0], gb[1], gb[2], gb[3], gb[4], c_ptr, gc[0], c.m, c.n, c.k, c.nkb,
                                     c.batch, c.batch2, int(c.bf), *[C.byref(o) for o in out])
    return st, dict(zip(F32_NAMES, (o.value for o in out)))


def _run_f32(c):
    _lib, L = _api()
    inp = _f32_inputs(c)
    ga, gb, gc = _f32_geometry(c)
    dt, odt = (BF if c.bf else torch.float32), (BF if c.out_bf else torch.float32)
    es = 2 if c.bf else 4
    shape_a, shape_b = (c.batch, c.batch2, c.nkb, c.m, c.k), (c.batch, c.batch2, c.nkb, c.k, c.n)
    fa, fb = torch.full((ga[5],), NAN, dtype=dt), torch.full((gb[5],), NAN, dtype=dt)
    fa[_index(shape_a, (ga[2], ga[3], ga[4], ga[0], ga[1]), c.a_off)] = inp["a"].reshape(-1)
    fb[_index(shape_b, (gb[2], gb[3], gb[4], gb[0], gb[1]), c.b_off)] = inp["b"].reshape(-1)
    ldc, sc, sc2, c_size = gc
    cidx = _index((c.batch, c.batch2, c.m, c.n), (sc, sc2, ldc, 1), 0)
    fc = _sentinel(1, c_size, odt).view(-1)
    if c.beta:
        fc[cidx.cuda()] = inp["c_old"].reshape(-1).cuda()
    fa, fb = fa.cuda(), fb.cuda()
    bias = inp["bias"].cuda() if c.bias else None
    a_ptr, b_ptr = fa.data_ptr() + es * c.a_off, fb.data_ptr() + es * c.b_off
    st, q = _f32_query(L, c, a_ptr, b_ptr, fc.data_ptr(), ga, gb, gc)
    want = dict(a_kc=int(c.a_kc), b_kc=int(c.b_kc), vec_a=c.vec[0], vec_b=c.vec[1], grid_x=((c.m + 127) // 128) * ((c.n + 127) // 128),
                grid_z=c.batch * c.batch2, stages=(c.k + 15) // 16)
    assert st == 0 and q == want, (c.name, st, q, want)
    bp = bias.data_ptr() if c.bias else None
    if c.b2:
        st = L.ts_gemm_f32_b2(a_ptr, ga[0], ga[1], ga[2], ga[3], ga[4], b_ptr, gb[0], gb[1], gb[2], gb[3], gb[4], fc.data_ptr(), ldc, sc, sc2, bp, c.m, c.n,
                              c.k, c.nkb, c.batch, c.batch2, int(c.beta), _stream())
    else:
        assert c.batch2 == 1
        st = L.ts_gemm_f32(a_ptr, ga[0], ga[1], ga[2], ga[4], b_ptr, gb[0], gb[1], gb[2], gb[4], fc.data_ptr(), ldc, sc, bp, c.m, c.n, c.k, c.nkb, c.batch,
                           int(c.bf), int(c.out_bf), int(c.beta), _stream())
    assert st == 0, (c.name, st)
    torch.cuda.synchronize()
    untouched = torch.ones(c_size, dtype=torch.bool, device="cuda")
    untouched[cidx.cuda()] = False
    assert bool((_bits(fc)[untouched] == (S16 if c.out_bf else S32)).all()), f"{c.name}: written outside [0, M) x [0, n) of a batch"
    v, bound = _f32_reference(c, inp)
    _assert_within(fc[cidx.cuda()].view(c.batch, c.batch2, c.m, c.n), v, bound, c.name, "gemm_f32 bf16" if c.out_bf else "gemm_f32 f32")


@gpu
@pytest.mark.parametrize("case", F32_LAYOUTS, ids=lambda c: c.name)
def test_f32_layouts_and_fetch_paths(case):
    _run_f32(case)


@gpu
@pytest.mark.parametrize("case", F32_OUTER, ids=lambda c: c.name)
def test_f32_outer_loop_with_a_partial_stage_in_every_step(case):
    _run_f32(case)


@gpu
@pytest.mark.parametrize("case", F32_BATCH2, ids=lambda c: c.name)
def test_f32_two_batch_levels(case):
    _run_f32(case)


@gpu
@pytest.mark.parametrize("case", F32_EPILOGUE, ids=lambda c: c.name)
def test_f32_epilogue_combinations(case):
    _run_f32(case)


def test_f32_table_covers_every_instantiation_and_path():
    """The layout table as the issue states it: each of the eight instantiations has a full-stage vector row, a K-tail row and an element-path row."""
    for bf in (False, True):
        for a_kc in (True, False):
            for b_kc in (True, False):
                rows = [c for c in F32_LAYOUTS if (c.bf, c.a_kc, c.b_kc) == (bf, a_kc, b_kc)]
                assert any(c.vec == (1, 1) and c.k % 16 == 0 for c in rows) and any(c.vec == (1, 1) and c.k % 16 for c in rows)
                assert any(0 in c.vec for c in rows)
    assert {c.m for c in F32_LAYOUTS} | {c.n for c in F32_LAYOUTS} == {1, 31, 33, 127, 128, 129} and {c.k for c in F32_LAYOUTS} == {1, 2, 15, 16, 17, 33}


def test_f32_refusals_and_paths_through_the_query():
    """No launch, no device: the refusals of gemm_f32_b2 and the conditions of the two fetch paths."""
    _lib, L = _api()
    E, U = _lib.TS_EINVAL, _lib.TS_EUNSUPPORTED
    base = dict(a=1 << 20, a_rs=24, a_cs=1, sa=4000, sa2=400, ska=40, b=2 << 20, b_rs=40, b_cs=1, sb=8000, sb2=800, skb=80, c=3 << 20, ldc=41, m=70, n=36, k=24,
                nkb=1, batch=2, batch2=3, bf=0)
    order = ("a", "a_rs", "a_cs", "sa", "sa2", "ska", "b", "b_rs", "b_cs", "sb", "sb2", "skb", "c", "ldc", "m", "n", "k", "nkb", "batch", "batch2", "bf")

    def ask(**kw):
        a = {**base, **kw}
        out = [C.c_int32(-7) for _ in F32_NAMES]
        st = L.ts_gemm_f32_launch_config(*[a[name] for name in order], *[C.byref(o) for o in out])
        return st, dict(zip(F32_NAMES, (o.value for o in out)))

    assert ask() == (0, dict(a_kc=1, b_kc=0, vec_a=1, vec_b=1, grid_x=1, grid_z=6, stages=2))
    assert ask(m=129, n=257, k=33, b_rs=260, ldc=260) == (0, dict(a_kc=1, b_kc=0, vec_a=1, vec_b=1, grid_x=6, grid_z=6, stages=3))
    for kw, vec in ((dict(a_rs=25), (0, 1)), (dict(sa=4001), (0, 1)), (dict(sa2=402), (0, 1)), (dict(ska=41), (0, 1)), (dict(a=(1 << 20) + 4), (0, 1)),
                    (dict(b_rs=42), (1, 0)), (dict(sb=8002), (1, 0)), (dict(sb2=801), (1, 0)), (dict(skb=83), (1, 0)), (dict(b=(2 << 20) + 8), (1, 0)),
                    (dict(bf=1, a=(1 << 20) + 8, b=(2 << 20) + 4), (1, 0)), (dict(bf=1, a=(1 << 20) + 2), (0, 1))):
        st, q = ask(**kw)
        assert st == 0 and (q["vec_a"], q["vec_b"]) == vec, (kw, st, q)
    assert ask(a_rs=1, a_cs=24, b_rs=1, b_cs=24)[1]["a_kc"] == 0 and ask(a_rs=1, a_cs=24, b_rs=1, b_cs=24)[1]["b_kc"] == 1
    st, q = ask(batch=256, batch2=256)                                                      # 65 536 grid z slices
    assert st == U and set(q.values()) == {-7}
    assert ask(batch=255, batch2=257)[0] == 0                                               # 65 535
    assert ask(a_rs=24, a_cs=2)[0] == U and ask(b_rs=40, b_cs=2)[0] == U                    # neither stride of an operand is 1
    for kw in (dict(a=None), dict(b=None), dict(c=None), dict(m=0), dict(n=0), dict(k=0), dict(nkb=0), dict(batch=0), dict(batch2=0), dict(ldc=35)):
        assert ask(**kw)[0] == E, kw
    out = [C.c_int32() for _ in F32_NAMES]
    for hole in range(len(out)):
        refs = [None if i == hole else C.byref(o) for i, o in enumerate(out)]
        assert L.ts_gemm_f32_launch_config(*[base[name] for name in order], *refs) == E


# =====================================================================================================================
# the bounds themselves, on the host
# =====================================================================================================================
def _nt_rows():
    """(name, inputs, use_bias, act, residual) of every gemm_nt row with a bound."""
    for ks in PIPELINE_KS:
        for act in (0, 2):
            yield f"pipeline K/32={ks} act={act}", _nt_inputs(257, 64, 32 * ks, 1000 + ks), True, act, False
    for m in ROW_EDGE_M:
        for n in (32, 96):
            yield f"rows M={m} N={n}", _nt_inputs(m, n, 64, 2000 + 10 * m + n), True, 0, False
    for act in (0, 1, 2):
        for use_bias in (True, False):
            for use_res in (False, True):
                yield f"epilogue act={act} bias={int(use_bias)} res={int(use_res)}", _nt_inputs(300, 96, 64, 3000), use_bias, act, use_res
    for kernel, stride in CONV:
        for act in (0, 1):
            yield f"conv kernel={kernel} act={act}", _conv_inputs(kernel, stride), True, act, False


def _f32_host(z, act):
    return torch.nn.functional.gelu(z) if act == 1 else (torch.nn.functional.silu(z) if act == 2 else z)


def test_bounds_admit_f32_arithmetic_and_are_not_vacuous():
    """torch's float32 CPU product of the same operands, with the same epilogue in f32, stays inside every bound: none is tighter than f32
    arithmetic allows.  And the median bound of each bf16 result is a small multiple of the bare rounding term u16 |y|: none is vacuous."""
    worst_multiple = 0.0
    for name, inp, use_bias, act, use_res in _nt_rows():
        v, b32, b16 = _nt_reference(inp, use_bias, act, use_res)
        x32 = inp.get("x2d", inp["x"]).float()                                    # the conv rows: the im2col matrix of the clips
        y = x32 @ inp["w"].float().t()
        if use_bias:
            y = y + inp["bias"]
        y = _f32_host(y, act)
        if use_res:
            y = y + inp["res"]
        assert bool(((y.double() - v).abs() <= b32).all()), name
        assert bool(((y.to(BF).double() - v).abs() <= b16).all()), name
        multiple = float(b16.median() / (U16 * v.abs()).median())
        worst_multiple = max(worst_multiple, multiple)
        assert multiple <= 1.5, (name, multiple)
    for rows, n, k, splits in SPLITK:
        inp = _splitk_inputs(rows, n, k, splits)
        e_parts, e_sum = _splitk_bounds(inp, k, splits)
        ks = k // splits
        parts = torch.stack([inp["x"].float()[:, z * ks:(z + 1) * ks] @ inp["w"].float()[:, z * ks:(z + 1) * ks].t() for z in range(splits)])
        assert bool(((parts.double() - inp["parts"]).abs() <= e_parts).all()), (rows, n, k, splits)
        total = parts[0].clone()
        for z in range(1, splits):
            total = total + parts[z]
        assert bool(((total.double() - inp["parts"].sum(0)).abs() <= e_sum).all()), (rows, n, k, splits)
    for n_mt, n_nt, _ in WALK[5:8]:                                              # the exact rows: f32 arithmetic IS exact there
        inp = _nt_exact_inputs((n_mt - 1) * 128 + 37, 256 * n_nt, 32, 4000 + 100 * n_mt + n_nt)
        assert torch.equal((inp["x"].float() @ inp["w"].float().t() + inp["bias"]).double(), inp["acc"] + inp["bias"].double())
    for c in F32_ALL:
        inp = _f32_inputs(c)
        v, bound = _f32_reference(c, inp)
        y = torch.einsum("xyjmk,xyjkn->xymn", inp["a"].float(), inp["b"].float())
        if c.bias:
            y = y + inp["bias"]
        if c.beta:
            y = y + inp["c_old"].float()
        if c.out_bf:
            y = y.to(BF)
            multiple = float(bound.median() / (U16 * v.abs()).median())
            worst_multiple = max(worst_multiple, multiple)
            assert multiple <= 1.5, (c.name, multiple)
        assert bool(((y.double() - v).abs() <= bound).all()), c.name
    print(f"[gemm-check] median bound of a bf16 result / median u16 |y|: at most {worst_multiple:.3f}")
