"""The data-path, text and augmentation kernels of csrc/misc.hip, csrc/dataprep.hip (collate), csrc/metrics.hip, csrc/augment.hip and the gradient wire
format of csrc/train.hip, each called by name through the C ABI with raw pointers and compared, element by element and bit for bit, with a restatement
written here in numpy / torch on the CPU (nothing of thunder_speech_amd or oracle takes part in the arithmetic).  The bounded kernels (AdamW, audio
prep, decoder gradient) are in tests/test_gpu_data_text_optim_bounded_kernels.py; tests/test_data_text_optim_restatements_host.py pins the restatements
of both files against tests/golden/r2_misc.npz and oracle/ on a machine without a GPU.

Entry point              kind of check   restatement
  ts_pack_activation     bit-equal       x.to(bfloat16) on the CPU (round to nearest even), 0 from min(t, max(len, 0)) to the pitch; NaN stays NaN
  ts_unpack_activation   bit-equal       bits << 16, every one of the 65536 bf16 patterns; the pitch padding (9.0) is never read into the result
  ts_grad_wire_pack      bit-equal       (g * f32(scale)).to(bfloat16); elements behind n untouched; NaN stays NaN, Inf keeps its sign
  ts_grad_wire_unpack    bit-equal       bits << 16; elements behind n untouched
  ts_im2col_time         bit-equal       numpy gather: out[(b k + u) C + c][t] = x[b][c][t s + u d - p] inside [0, min(t_in, max(len, 0))), else 0
  ts_lengths_map         bit-equal       torch.div(l + add, div, rounding_mode="floor") + plus in the input dtype, cast to the output dtype
  ts_collate_pad         bit-equal       row i = clip i followed by zeros
  ts_edit_distance       equal           numpy two-row Levenshtein dynamic programme
  ts_encode_chars        equal           dictionary lookup, start / end ids, pad_id
  ts_spec_mask_apply     bit-equal       masked_fill of the rectangle [f0, f1) x [t0, t1) per table row
  ts_spec_masks_draw     equal           Philox4x32-10 restated in numpy integers, the span arithmetic in stepwise float32

Conventions as in tests/test_gpu_frontend_kernels.py and tests/test_gpu_tcs_kernels.py: return codes asserted; outputs inside NaN-filled (integers:
sentinel-filled) buffers between guards that must come back bit for bit; `RATIO|kind|mismatching elements` printed before every assert (an exact
check has bound 0: the figure is the number of elements that differ, and it must be 0); no element left out.

Boundary probing of ts_spec_masks_draw: a device / restatement disagreement in (int)(u (size - value)) can only show where min_value lies next to an
integer.  For draws spread over more than a few units the share of spans with min_value within 1e-3 of an integer is 2e-3 whatever the widths; it
only rises where size - value is itself small (size 1: 1e-3 (1 + ln 1000) = 0.8 %).  1 % per launch is therefore out of reach of any choice of widths
at the three geometries (the host test computes the shares from the restatement alone: 0.11 % .. 0.79 %); every launch is asserted to hold at least
1e-3 of its 8000 spans there (half the 2e-3 that uniform draws give), and the sweep as a whole more than 300 such spans.  That a one-ulp difference
in size - value is seen is shown by two seeds searched for with the restatement (DRAW_SEEDS)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")
BF = torch.bfloat16
GUARD = 7.0
PAD = 9.0
G = 64                                    # guard elements in front of and behind a flat output (a multiple of 16 bytes in every element size)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _exact(kind, what, got, want):
    """bit / value equality of two CPU tensors of one shape and dtype; prints the number of elements that differ"""
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype} against {want.shape} {want.dtype}"
    bad = got != want
    n = int(bad.sum())
    print(f"RATIO|{kind}|{float(n):.3e}|{what}")
    if n:
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{what}: {n} of {bad.numel()} elements differ, first at flat index {i}: got {got.flatten()[i].item()} want {want.flatten()[i].item()}")


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _flat(n, dtype, fill, guard):
    """-> (buffer, view of n elements between G guard elements); float fills may be NaN"""
    buf = torch.full((n + 2 * G,), fill, dtype=dtype, device="cuda")
    buf[:G] = guard
    buf[G + n:] = guard
    return buf, buf[G: G + n]


def _flat_ok(buf, n, guard, what):
    assert bool((buf[:G] == guard).all()) and bool((buf[G + n:] == guard).all()), f"{what}: a guard element next to the output was written"


def _rows(rows, pitch, dtype, guard_rows=4):
    buf = torch.full((rows + 2 * guard_rows, pitch), NAN, dtype=dtype, device="cuda")
    buf[:guard_rows] = GUARD
    buf[guard_rows + rows:] = GUARD
    return buf, buf[guard_rows: guard_rows + rows]


def _rows_ok(buf, rows, what, guard_rows=4):
    assert bool((torch.cat([buf[:guard_rows], buf[guard_rows + rows:]]) == GUARD).all()), f"{what}: a guard row next to the output was written"


def _r8(x):
    return (x + 7) // 8 * 8


# ---------------------------------------------------------------------------------------------------------------------
# adversarial float32 values for the two bf16 roundings
# ---------------------------------------------------------------------------------------------------------------------
def adversarial_f32():
    """ties in both directions (to even), next to ties, the largest finite f32 (rounds to Inf), +-Inf, quiet / signalling-pattern / negative NaN, +-0, f32
    denormals, the smallest bf16 denormal +-, half of it (a tie to 0) and just above (rounds up to it), the largest values that stay finite"""
    pos = [0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0x3F817FFF, 0x3F818001, 0x7F7FFFFF, 0x7F7F7FFF, 0x7F7F8000, 0x7F800000, 0x00000000, 0x00000001,
           0x007FFFFF, 0x00400000, 0x00010000, 0x00008000, 0x00008001, 0x00007FFF, 0x00018000, 0x00800000, 0x00808000, 0x3EAAAAAB, 0x40490FDB]
    nan = [0x7FC00000, 0x7F800001, 0x7FA00000, 0xFFC00000, 0xFF800001, 0x7FFFFFFF]
    words = pos + [w | 0x80000000 for w in pos] + nan
    return torch.from_numpy(np.array(words, dtype=np.uint32).view(np.float32).copy())


def bf16_round_bits(x):
    """f32 CPU tensor -> (int16 bits of x.to(bfloat16) as torch rounds on the CPU, mask of the NaN elements)"""
    return _bits(x.to(BF)), torch.isnan(x)


def _check_rounded(kind, what, got_bits, x, fill_bits=None):
    """got_bits int16 against torch's CPU rounding of x: bit-equal where x is no NaN; NaN where it is (and not the buffer's fill pattern)"""
    want, nan = bf16_round_bits(x)
    got_f = got_bits.view(BF).float()
    assert bool(torch.isnan(got_f[nan]).all()), f"{what}: a NaN came out as a number"
    if fill_bits is not None and bool(nan.any()):
        assert bool((got_bits[nan] != fill_bits).all()), f"{what}: a NaN element was not written"
    inf = torch.isinf(x)
    assert bool((got_f[inf] == x[inf]).all()), f"{what}: an infinity lost its sign or became finite"
    _exact(kind, what, torch.where(nan, torch.zeros_like(got_bits), got_bits), torch.where(nan, torch.zeros_like(want), want))


# ---------------------------------------------------------------------------------------------------------------------
# 1. ts_pack_activation / ts_unpack_activation
# ---------------------------------------------------------------------------------------------------------------------
def pack_reference(x, lens, pitch):
    """x f32 [b][c][t], lens list or None -> f32 [b][c][pitch] whose bf16 rounding is the expected result (0 from the limit to the pitch)"""
    b, c, t = x.shape
    out = torch.zeros(b, c, pitch)
    for i in range(b):
        lim = t if lens is None else min(t, max(int(lens[i]), 0))
        out[i, :, :lim] = x[i, :, :lim]
    return out


def _run_pack(L, x, lens, pitch, what):
    b, c, t = x.shape
    xd = x.cuda().contiguous()
    ld = torch.tensor(lens, dtype=torch.int32).cuda() if lens is not None else None
    buf, dst = _rows(b * c, pitch, BF)
    assert L.ts_pack_activation(xd.data_ptr(), ld.data_ptr() if ld is not None else None, b, c, t, dst.data_ptr(), pitch, _stream()) == 0, what
    torch.cuda.synchronize()
    _rows_ok(buf, b * c, what)
    return _bits(dst.cpu()).view(b, c, pitch)


@pytest.mark.parametrize("b,c,t,pitch", [(1, 1, 1, 8), (2, 3, 7, 8), (2, 5, 8, 16), (3, 4, 9, 16), (2, 64, 257, 264), (1, 2, 1001, 1008)])
def test_pack_activation_is_torchs_bf16_rounding_with_a_zero_tail(b, c, t, pitch):
    from thunder_speech_amd import _lib
    L = _lib.lib()
    x = torch.randn(b, c, t, generator=torch.Generator().manual_seed(t)) * 3.0
    edge = [0, 1, t - 1, t, t + 5, -3]
    variants = [None] + [[edge[(s + i) % 6] for i in range(b)] for s in range(0, 6, b)]
    assert {v for lens in variants[1:] for v in lens} == set(edge)
    for lens in variants:
        what = f"pack b={b} c={c} t={t} pitch={pitch} lens={lens}"
        got = _run_pack(L, x, lens, pitch, what)
        _check_rounded("pack", what, got, pack_reference(x, lens, pitch))


def test_pack_activation_rounds_adversarial_values_like_torch():
    from thunder_speech_amd import _lib
    L = _lib.lib()
    adv = adversarial_f32()
    t = adv.numel() + 3
    x = torch.randn(2, 3, t, generator=torch.Generator().manual_seed(1))
    x[0, 0, :adv.numel()] = adv
    x[0, 2, 3:] = adv                                   # another position inside the 8-element groups
    x[1, 1, :adv.numel()] = adv.flip(0)
    for lens in (None, [t, t - 2]):
        what = f"pack adversarial lens={lens}"
        got = _run_pack(L, x, lens, _r8(t), what)
        _check_rounded("pack-adversarial", what, got, pack_reference(x, lens, _r8(t)))


def test_unpack_activation_widens_every_bf16_pattern_and_skips_the_padding():
    from thunder_speech_amd import _lib
    L = _lib.lib()
    for b, c, t, pitch in [(1, 64, 1024, 1032), (2, 3, 7, 8), (3, 4, 9, 16), (1, 1, 1, 8), (1, 2, 1001, 1001)]:
        what = f"unpack b={b} c={c} t={t} pitch={pitch}"
        n = b * c * t
        pat = torch.arange(n, dtype=torch.int64) * (1 if n >= 65536 else 7919) % 65536          # the bf16 patterns as unsigned numbers
        signed = pat - 65536 * (pat >= 32768)
        src = torch.full((b * c, pitch), PAD, dtype=BF)
        _bits(src)[:, :t] = signed.view(b * c, t).to(torch.int16)
        sd = src.cuda()
        buf, dst = _flat(n, torch.float32, 0.0, GUARD)
        _bits(dst).fill_(0x7FC12345)                    # a NaN that no widened bf16 equals
        assert L.ts_unpack_activation(sd.data_ptr(), b, c, t, pitch, dst.data_ptr(), _stream()) == 0, what
        torch.cuda.synchronize()
        _flat_ok(buf, n, GUARD, what)
        _exact("unpack", what, _bits(dst.cpu()), (signed << 16).to(torch.int32))
        if n >= 65536:
            assert len(set(pat.tolist())) == 65536


def test_pack_and_unpack_refuse_what_they_document():
    from thunder_speech_amd import _lib
    L, E = _lib.lib(), _lib.TS_EINVAL
    a = torch.zeros(4096, device="cuda").data_ptr()
    assert L.ts_pack_activation(a, None, 1, 2, 9, a, 16, None) == 0
    for args in [(a, None, 1, 2, 9, a, 12), (a, None, 1, 2, 9, a, 8), (None, None, 1, 2, 9, a, 16), (a, None, 1, 2, 9, None, 16), (a, None, 0, 2, 9, a, 16),
                 (a, None, 1, 0, 9, a, 16), (a, None, 1, 2, 0, a, 16)]:
        assert L.ts_pack_activation(*args, None) == E, args
    assert L.ts_unpack_activation(a, 1, 2, 9, 16, a, None) == 0
    for args in [(a, 1, 2, 9, 8, a), (None, 1, 2, 9, 16, a), (a, 1, 2, 9, 16, None), (a, 0, 2, 9, 16, a), (a, 1, 0, 9, 16, a), (a, 1, 2, 0, 16, a)]:
        assert L.ts_unpack_activation(*args, None) == E, args
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# 2. ts_grad_wire_pack / ts_grad_wire_unpack
# ---------------------------------------------------------------------------------------------------------------------
WIRE_FILL = 0x7FD5                        # a bf16 NaN that no rounding produces


def wire_reference(g, scale):
    return g * torch.tensor(scale, dtype=torch.float32)


@pytest.mark.parametrize("n", [1, 7, 8, 9, 2047, 2048 * 256 * 8 + 13])
def test_grad_wire_round_trip_is_bit_exact_and_stays_inside_n(n):
    from thunder_speech_amd import _lib
    L = _lib.lib()
    adv = adversarial_f32()
    g = torch.randn(n, generator=torch.Generator().manual_seed(n)) * 2.0
    k = min(n, adv.numel())
    g[:k] = adv[:k]
    g[n - k:] = adv[adv.numel() - k:]                   # the tail elements (n & 7) and, at the largest n, the wrapped part of the grid-stride loop
    if n > 4 * adv.numel():
        mid = (2048 * 256 * 8 if n > 2048 * 256 * 8 else n // 2) - 26         # across the end of the grid's first pass
        g[mid: mid + adv.numel()] = adv[:n - mid]
    gd = g.cuda()
    for scale in (1.0, 0.125, 1.0 / 3.0):
        what = f"grad wire n={n} scale={scale}"
        wbuf, wire = _flat(n, BF, 0.0, GUARD)
        _bits(wire).fill_(WIRE_FILL)
        assert L.ts_grad_wire_pack(gd.data_ptr(), wire.data_ptr(), n, scale, _stream()) == 0, what
        torch.cuda.synchronize()
        _flat_ok(wbuf, n, GUARD, what + " pack")
        got = _bits(wire.cpu())
        _check_rounded("grad-wire-pack", what, got, wire_reference(g, scale), fill_bits=WIRE_FILL)
        bbuf, back = _flat(n, torch.float32, 0.0, GUARD)
        _bits(back).fill_(0x7FC12345)
        assert L.ts_grad_wire_unpack(wire.data_ptr(), back.data_ptr(), n, _stream()) == 0, what
        torch.cuda.synchronize()
        _flat_ok(bbuf, n, GUARD, what + " unpack")
        _exact("grad-wire-unpack", what, _bits(back.cpu()), got.to(torch.int32) << 16)
    # the largest finite f32 survives the product with 1.0 and overflows only in the rounding
    assert float(wire_reference(adv[6:7], 1.0)) == float(adv[6]) and bool(torch.isinf(adv[6:7].to(BF)).all())


def test_grad_wire_refuses_misaligned_and_null_pointers():
    from thunder_speech_amd import _lib
    L, E = _lib.lib(), _lib.TS_EINVAL
    g = torch.zeros(64, device="cuda")
    w = torch.zeros(64, dtype=BF, device="cuda")
    gp, wp = g.data_ptr(), w.data_ptr()
    assert L.ts_grad_wire_pack(gp, wp, 9, 1.0, None) == 0 and L.ts_grad_wire_unpack(wp, gp, 9, None) == 0
    for a, b in [(gp + 4, wp), (gp, wp + 2), (gp + 8, wp), (gp, wp + 8), (None, wp), (gp, None)]:
        assert L.ts_grad_wire_pack(a, b, 9, 1.0, None) == E and L.ts_grad_wire_unpack(b, a, 9, None) == E, (a, b)
    assert L.ts_grad_wire_pack(gp, wp, 0, 1.0, None) == E and L.ts_grad_wire_unpack(wp, gp, 0, None) == E
    torch.cuda.synchronize()
    assert bool((g == 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# 3. ts_im2col_time
# ---------------------------------------------------------------------------------------------------------------------
def conv_t_out(t_in, k, stride, dil, pad):
    return (t_in + 2 * pad - dil * (k - 1) - 1) // stride + 1


def im2col_reference(x, lens, t_in, k, stride, dil, pad, t_out, pitch_out):
    """x int16 numpy [b][C][pitch_in] -> int16 [b][k][C][pitch_out]"""
    b, ch, _ = x.shape
    out = np.zeros((b, k, ch, pitch_out), dtype=np.int16)
    t = np.arange(t_out)
    for i in range(b):
        lim = t_in if lens is None else min(t_in, max(int(lens[i]), 0))
        for u in range(k):
            ti = t * stride + u * dil - pad
            ok = (ti >= 0) & (ti < lim)
            out[i, u, :, :t_out] = np.where(ok[None, :], x[i][:, np.clip(ti, 0, t_in - 1)], 0)
    return out


@pytest.mark.parametrize("k,stride,dil,pad,t_in", [(1, 1, 1, 0, 9), (3, 1, 1, 1, 8), (5, 2, 1, 2, 17), (11, 3, 1, 5, 40), (3, 1, 2, 2, 16), (7, 2, 3, 20, 33),
                                                   (33, 1, 1, 16, 5)])
def test_im2col_time_is_a_gather_with_zero_fill(k, stride, dil, pad, t_in):
    from thunder_speech_amd import _lib
    L = _lib.lib()
    full = conv_t_out(t_in, k, stride, dil, pad)
    assert full >= 4
    pitch_in = t_in + 3
    gen = torch.Generator().manual_seed(k * 100 + t_in)
    n_bad = 0
    for ch in (1, 5):
        for b in (1, 3):
            x = (torch.randn(b, ch, pitch_in, generator=gen) + 4.0).to(BF)           # no zeros: a zero in the result is a fill
            _bits(x)[:, :, t_in:] = 0x7FC0                                           # NaN in the padding of the input rows
            xd = x.cuda()
            xn = _bits(x).numpy()
            ragged = [t_in, t_in // 2, 1][:b] if b > 1 else [t_in // 2]
            for lens in (None, [t_in] * b, [0] * b, [1] * b, ragged, [t_in + 5] * b, [-3] * b):
                ld = torch.tensor(lens, dtype=torch.int32).cuda() if lens is not None else None
                for t_out in (full, full - 3):
                    for pitch_out in (_r8(t_out), _r8(t_out) + 8):
                        what = f"im2col k={k} s={stride} d={dil} p={pad} t_in={t_in} C={ch} b={b} lens={lens} t_out={t_out} pitch_out={pitch_out}"
                        rows = b * k * ch
                        buf, out = _rows(rows, pitch_out, BF)
                        st = L.ts_im2col_time(xd.data_ptr(), ld.data_ptr() if ld is not None else None, out.data_ptr(), b, ch, t_in, pitch_in, k, stride, dil,
                                              pad, t_out, pitch_out, _stream())
                        assert st == 0, what
                        torch.cuda.synchronize()
                        _rows_ok(buf, rows, what)
                        got = _bits(out.cpu()).numpy().reshape(b, k, ch, pitch_out)
                        want = im2col_reference(xn, lens, t_in, k, stride, dil, pad, t_out, pitch_out)
                        bad = int((got != want).sum())
                        n_bad += bad
                        assert bad == 0, f"{what}: {bad} elements differ"
    print(f"RATIO|im2col|{float(n_bad):.3e}|k={k} s={stride} d={dil} p={pad} t_in={t_in}")
    a = torch.zeros(4096, device="cuda").data_ptr()
    E = _lib.TS_EINVAL
    assert L.ts_im2col_time(a, None, a, 1, 1, 9, 9, 3, 1, 1, 1, 9, 12, None) == E and L.ts_im2col_time(a, None, a, 1, 1, 9, 9, 3, 1, 1, 1, 9, 8, None) == E
    assert L.ts_im2col_time(a, None, a, 1, 1, 9, 8, 3, 1, 1, 1, 9, 16, None) == E and L.ts_im2col_time(None, None, a, 1, 1, 9, 9, 3, 1, 1, 1, 9, 16, None) == E
    assert L.ts_im2col_time(a, None, None, 1, 1, 9, 9, 3, 1, 1, 1, 9, 16, None) == E and L.ts_im2col_time(a, None, a, 1, 1, 9, 9, 3, 0, 1, 1, 9, 16, None) == E


# ---------------------------------------------------------------------------------------------------------------------
# 4. ts_lengths_map
# ---------------------------------------------------------------------------------------------------------------------
KINDS = {0: torch.float32, 1: torch.int64, 2: torch.int32}
CONV_GEOMETRIES = [(33, 2, 1, 16), (87, 1, 2, 86), (11, 3, 1, 5), (1, 1, 1, 0)]
TRIPLES = [(0, 160, 1)] + [(2 * p - d * (k - 1) - 1, s, 1) for k, s, d, p in CONV_GEOMETRIES] + [(-7, 3, 0)]
INT_ONLY_TRIPLES = [(5, -2, 0)]


def lengths_reference(x, add, div, plus, out_kind):
    return (torch.div(x + add, div, rounding_mode="floor") + plus).to(KINDS[out_kind])


def lengths_inputs(in_kind):
    ints = torch.arange(-50, 4101)
    if in_kind == 0:
        return torch.cat([ints.float(), ints.float() + 0.5])
    return ints.to(KINDS[in_kind])


def _run_lengths(L, x, in_kind, out_kind, add, div, plus, with_out=True, with_i32=True):
    n = x.numel()
    xd = x.cuda()
    obuf, out = _flat(n, KINDS[out_kind], NAN if out_kind == 0 else -7777, -7)
    ibuf, o32 = _flat(n, torch.int32, -7777, -7)
    st = L.ts_lengths_map(xd.data_ptr(), in_kind, out.data_ptr() if with_out else None, out_kind, o32.data_ptr() if with_i32 else None, n, add, div, plus,
                          _stream())
    torch.cuda.synchronize()
    what = f"lengths_map in={in_kind} out={out_kind} n={n} ({add}, {div}, {plus})"
    assert st == 0, what
    _flat_ok(obuf, n, -7, what)
    _flat_ok(ibuf, n, -7, what)
    return out.cpu(), o32.cpu(), what


@pytest.mark.parametrize("in_kind", [0, 1, 2])
@pytest.mark.parametrize("out_kind", [0, 1, 2])
def test_lengths_map_is_torchs_floor_division_in_the_input_dtype(in_kind, out_kind):
    from thunder_speech_amd import _lib
    L = _lib.lib()
    x = lengths_inputs(in_kind)
    for add, div, plus in TRIPLES + (INT_ONLY_TRIPLES if in_kind else []):
        got, got32, what = _run_lengths(L, x, in_kind, out_kind, add, div, plus)
        _exact("lengths-map", what, got, lengths_reference(x, add, div, plus, out_kind))
        _exact("lengths-map-i32", what, got32, lengths_reference(x, add, div, plus, 2))
    for n in (1, 255, 256, 257):
        xs = x[1000: 1000 + n].contiguous()
        got, got32, what = _run_lengths(L, xs, in_kind, out_kind, 0, 160, 1)
        _exact("lengths-map", what, got, lengths_reference(xs, 0, 160, 1, out_kind))
        _exact("lengths-map-i32", what, got32, lengths_reference(xs, 0, 160, 1, 2))
    # one output only: the other stays as it was
    xs = x[:257].contiguous()
    got, got32, what = _run_lengths(L, xs, in_kind, out_kind, -7, 3, 0, with_i32=False)
    _exact("lengths-map", what, got, lengths_reference(xs, -7, 3, 0, out_kind))
    assert bool((got32 == -7777).all())
    got, got32, what = _run_lengths(L, xs, in_kind, out_kind, -7, 3, 0, with_out=False)
    _exact("lengths-map-i32", what, got32, lengths_reference(xs, -7, 3, 0, 2))
    assert bool(torch.isnan(got).all()) if out_kind == 0 else bool((got == -7777).all())


def test_lengths_map_refuses_what_it_documents():
    from thunder_speech_amd import _lib
    L, E = _lib.lib(), _lib.TS_EINVAL
    a = torch.zeros(64, device="cuda").data_ptr()
    assert L.ts_lengths_map(a, 0, a, 0, None, 4, 0, 160, 1, None) == 0
    for args in [(a, 0, a, 0, None, 4, 0, 0, 1), (a, 3, a, 0, None, 4, 0, 160, 1), (a, -1, a, 0, None, 4, 0, 160, 1), (a, 0, a, 3, None, 4, 0, 160, 1),
                 (a, 0, a, -1, None, 4, 0, 160, 1), (a, 0, None, 0, None, 4, 0, 160, 1), (None, 0, a, 0, None, 4, 0, 160, 1), (a, 0, a, 0, None, 0, 0, 160, 1)]:
        assert L.ts_lengths_map(*args, None) == E, args
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# 5. ts_collate_pad
# ---------------------------------------------------------------------------------------------------------------------
def collate_reference(clips, max_len):
    out = torch.zeros(len(clips), max_len)
    for i, c in enumerate(clips):
        out[i, :c.numel()] = c
    return out


def collate_lengths(max_len, n_clips):
    k4 = max(max_len // 2, 1) // 4 * 4
    lens = [max_len, 1, k4, k4 + 1, k4 + 3]
    return [min(max(v, 1), max_len) for v in lens][:n_clips]


@pytest.mark.parametrize("max_len", [1, 3, 4, 7, 1024, 1027, 65536 + 4, 65536 + 5])
@pytest.mark.parametrize("n_clips", [1, 5])
def test_collate_pad_copies_each_clip_and_zero_fills(max_len, n_clips):
    from thunder_speech_amd import _lib
    L = _lib.lib()
    gen = torch.Generator().manual_seed(max_len)
    lens = collate_lengths(max_len, n_clips)
    for rot in range(4):                                # every clip meets every offset from 16-byte alignment: 0, 4, 8 and 12 bytes
        clips, keep, rows = [], [], []
        for i, n in enumerate(lens):
            off = (i + rot) % 4
            clip = torch.randn(n, generator=gen) + 3.0                                # no zeros, no 9.0
            alloc = torch.full((off + n + 8,), PAD, device="cuda")                    # the clip's own allocation: guard samples of 9.0 behind it
            alloc[off: off + n] = clip.cuda()
            assert alloc.data_ptr() % 16 == 0
            clips.append(clip)
            keep.append(alloc)
            rows.append([alloc.data_ptr() + 4 * off, n])
        table = torch.tensor(rows, dtype=torch.int64).cuda()
        buf, out = _flat(n_clips * max_len, torch.float32, NAN, GUARD)
        assert out.data_ptr() % 16 == 0
        what = f"collate n_clips={n_clips} max_len={max_len} lens={lens} rot={rot}"
        assert L.ts_collate_pad(table.data_ptr(), n_clips, max_len, out.data_ptr(), _stream()) == 0, what
        torch.cuda.synchronize()
        _flat_ok(buf, n_clips * max_len, GUARD, what)
        got = out.cpu().view(n_clips, max_len)
        assert not bool((got == PAD).any()), f"{what}: a sample from behind a clip's end reached the batch"
        _exact("collate", what, _bits(got), _bits(collate_reference(clips, max_len)))
    E = _lib.TS_EINVAL
    assert L.ts_collate_pad(None, 1, 4, out.data_ptr(), None) == E and L.ts_collate_pad(table.data_ptr(), 1, 4, None, None) == E
    assert L.ts_collate_pad(table.data_ptr(), 0, 4, out.data_ptr(), None) == E and L.ts_collate_pad(table.data_ptr(), 1, 0, out.data_ptr(), None) == E


# ---------------------------------------------------------------------------------------------------------------------
# 6. ts_edit_distance
# ---------------------------------------------------------------------------------------------------------------------
EDIT_LIMIT = 5460                         # 3 (n + 1) int32 of LDS <= 64 KiB


def edit_distance_reference(a, b):
    """Levenshtein distance, two-row dynamic programme; a row's insertions d[j] = min(d[j], d[j - 1] + 1) are a running minimum of d[j] - j"""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    j = np.arange(len(b) + 1, dtype=np.int64)
    prev = j.copy()
    for i in range(1, len(a) + 1):
        cur = np.empty_like(prev)
        cur[0] = i
        cur[1:] = np.minimum(prev[:-1] + (b != a[i - 1]), prev[1:] + 1)
        prev = np.minimum.accumulate(cur - j) + j
    return int(prev[-1])


def edit_pairs_small():
    r = np.random.Generator(np.random.PCG64(11))
    seq = lambda n, v: r.integers(0, v, n).tolist()
    big = [int(v) for v in r.integers(-2 ** 31, 2 ** 31 - 1, 40)] + [2 ** 30 + 1, 2 ** 31 - 1, -1, -2 ** 31]
    s300 = seq(300, 5)
    pairs = [([], []), ([], seq(5, 3)), (seq(5, 3), []), ([4], [4]), ([4], [5]), (seq(255, 4), seq(255, 4)), (seq(256, 4), seq(256, 4)), (seq(257, 3), seq(3, 3)),
             (seq(3, 3), seq(257, 3)), (seq(300, 6), seq(1100, 6)), (seq(1100, 6), seq(300, 6)), (s300, list(s300)), (s300, s300[::-1]), (s300, [9] + s300),
             (s300, s300 + [9]), ([9] + s300, s300), (big, big[::2] + [7]), (big, list(big)), (seq(700, 2), seq(650, 2))]
    return pairs


def edit_pairs_large():
    r = np.random.Generator(np.random.PCG64(12))
    seq = lambda n, v: r.integers(0, v, n).tolist()
    return [(seq(EDIT_LIMIT, 2), seq(EDIT_LIMIT, 2)), (seq(EDIT_LIMIT, 1000), seq(EDIT_LIMIT, 1000)), (seq(7, 50), seq(20000, 50)), ([], []), ([1], [2])]


def _flatten(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(s) for s in seqs])
    flat = np.array([v for s in seqs for v in s] + [0], dtype=np.int64).astype(np.int32)
    return torch.from_numpy(flat).cuda(), torch.from_numpy(off).cuda()


def _run_edit(L, pairs, max_a_len=None):
    a, a_off = _flatten([p[0] for p in pairs])
    b, b_off = _flatten([p[1] for p in pairs])
    buf, dist = _flat(len(pairs), torch.int32, -7777, -7)
    longest = max(len(p[0]) for p in pairs)
    st = L.ts_edit_distance(a.data_ptr(), a_off.data_ptr(), b.data_ptr(), b_off.data_ptr(), len(pairs), longest if max_a_len is None else max_a_len,
                            dist.data_ptr(), _stream())
    torch.cuda.synchronize()
    _flat_ok(buf, len(pairs), -7, "edit distance")
    return st, dist.cpu()


@pytest.mark.parametrize("which", ["small", "large"])
def test_edit_distance_matches_the_two_row_programme(which):
    from thunder_speech_amd import _lib
    L = _lib.lib()
    pairs = edit_pairs_small() if which == "small" else edit_pairs_large()
    longest = max(len(p[0]) for p in pairs)
    assert sum(len(p[0]) < longest for p in pairs) >= len(pairs) - 2              # max_a_len exceeds most pairs' n
    st, dist = _run_edit(L, pairs)
    assert st == 0
    want = torch.tensor([edit_distance_reference(*p) for p in pairs], dtype=torch.int32)
    _exact("edit-distance", f"{which}: (n, m) = {[(len(x), len(y)) for x, y in pairs]}", dist, want)


def test_edit_distance_refuses_sequences_beyond_its_lds():
    from thunder_speech_amd import _lib
    from thunder_speech_amd.metrics import edit_distances
    L = _lib.lib()
    pairs = [([1, 2, 3], [1, 3]), ([], [5])]
    st, dist = _run_edit(L, pairs, max_a_len=EDIT_LIMIT + 1)
    assert st == _lib.TS_EUNSUPPORTED and bool((dist == -7777).all())
    st, dist = _run_edit(L, pairs, max_a_len=EDIT_LIMIT)
    assert st == 0 and dist.tolist() == [1, 1]
    st, dist = _run_edit(L, pairs, max_a_len=-1)
    assert st == _lib.TS_EINVAL and bool((dist == -7777).all())
    with pytest.raises(NotImplementedError):
        edit_distances([[1] * (EDIT_LIMIT + 1)], [[1, 2]])
    assert edit_distances([[1, 2]], [[1] * (EDIT_LIMIT + 1)]).cpu().tolist() == [EDIT_LIMIT]      # the limit is on the prediction's side only


# ---------------------------------------------------------------------------------------------------------------------
# 7. ts_encode_chars
# ---------------------------------------------------------------------------------------------------------------------
def encode_reference(rows, vocab, unk_id, start_id, end_id, pad_id, s_max):
    out = np.full((len(rows), s_max), pad_id, dtype=np.int64)
    lens = np.zeros(len(rows), dtype=np.int64)
    for i, r in enumerate(rows):
        ids = ([start_id] if start_id >= 0 else []) + [vocab.get(cp, unk_id) for cp in r] + ([end_id] if end_id >= 0 else [])
        out[i, :len(ids)] = ids
        lens[i] = len(ids)
    return out, lens


def encode_vocab(n):
    """n sorted code points with gaps (some above 0xFFFF) -> non-contiguous ids"""
    cps = [40 + 3 * i for i in range(n)] if n <= 28 else [40 + 3 * i for i in range(n - 600)] + [0x10000 + 5 * i for i in range(600)]
    return {cp: (i * 7 + 3) % 100003 for i, cp in enumerate(cps)}


def encode_rows(vocab, seed):
    r = np.random.Generator(np.random.PCG64(seed))
    cps = sorted(vocab)
    lo, hi = (cps[0], cps[-1]) if cps else (40, 50)
    known = lambda n: [cps[int(i)] for i in r.integers(0, len(cps), n)] if cps else [45] * n
    return [known(11), [], known(3) + [lo - 1, 0, lo + 1, hi + 1, 0x10FFFF, hi - 1] + known(2), known(1), [], known(290), [lo, hi] if cps else [1, 2]]


@pytest.mark.parametrize("n_vocab", [0, 1, 28, 5000])
def test_encode_chars_is_a_dictionary_lookup_with_padding(n_vocab):
    from thunder_speech_amd import _lib
    L = _lib.lib()
    vocab = encode_vocab(n_vocab)
    rows = encode_rows(vocab, n_vocab)
    text, off = _flatten(rows)
    cps = sorted(vocab)
    vc = torch.tensor(cps + [0], dtype=torch.int32).cuda()
    vi = torch.tensor([vocab[c] for c in cps] + [0], dtype=torch.int32).cuda()
    n_bad = 0
    for start_id, end_id in [(100001, -1), (-1, 100002), (100001, 100002), (-1, -1)]:
        for pad_id, unk_id in [(0, 99), (-1, 7), (-123456, -5)]:
            longest = max(len(r) for r in rows) + (start_id >= 0) + (end_id >= 0)
            for s_max in (longest, longest + 300):
                what = f"encode n_vocab={n_vocab} start={start_id} end={end_id} pad={pad_id} unk={unk_id} s_max={s_max}"
                obuf, out = _flat(len(rows) * s_max, torch.int64, -7777, -7)
                lbuf, lens = _flat(len(rows), torch.int64, -7777, -7)
                st = L.ts_encode_chars(text.data_ptr(), off.data_ptr(), len(rows), vc.data_ptr() if n_vocab else None, vi.data_ptr() if n_vocab else None, n_vocab,
                                       unk_id, start_id, end_id, pad_id, s_max, out.data_ptr(), lens.data_ptr(), _stream())
                assert st == 0, what
                torch.cuda.synchronize()
                _flat_ok(obuf, len(rows) * s_max, -7, what)
                _flat_ok(lbuf, len(rows), -7, what)
                want, want_lens = encode_reference(rows, vocab, unk_id, start_id, end_id, pad_id, s_max)
                bad = int((out.cpu().numpy().reshape(len(rows), s_max) != want).sum()) + int((lens.cpu().numpy() != want_lens).sum())
                n_bad += bad
                assert bad == 0, f"{what}: {bad} elements differ"
    print(f"RATIO|encode-chars|{float(n_bad):.3e}|n_vocab={n_vocab}")
    E = _lib.TS_EINVAL
    a = out.data_ptr()
    assert L.ts_encode_chars(text.data_ptr(), None, 1, None, None, 0, 0, -1, -1, 0, 4, a, a, None) == E
    assert L.ts_encode_chars(text.data_ptr(), off.data_ptr(), 1, None, None, 3, 0, -1, -1, 0, 4, a, a, None) == E
    assert L.ts_encode_chars(text.data_ptr(), off.data_ptr(), 1, None, None, 0, 0, -1, -1, 0, 0, a, a, None) == E
    assert L.ts_encode_chars(text.data_ptr(), off.data_ptr(), 0, None, None, 0, 0, -1, -1, 0, 4, a, a, None) == E


# ---------------------------------------------------------------------------------------------------------------------
# 8. ts_spec_mask_apply
# ---------------------------------------------------------------------------------------------------------------------
def mask_reference(x, table):
    """x [B][C][t] -> copy with masked_fill(rectangle, 0) per row (f0, f1, t0, t1); a rectangle is the set f0 <= f < f1, t0 <= t < t1"""
    y = x.clone()
    f = torch.arange(x.shape[1])[:, None]
    t = torch.arange(x.shape[2])[None, :]
    for f0, f1, t0, t1 in table:
        y = y.masked_fill(((f >= f0) & (f < f1) & (t >= t0) & (t < t1))[None], 0.0)
    return y


MASK_TABLES = {
    "mixed": [(3, 3, 0, 50), (10, 5, 0, 50), (-4, 2, -6, 3), (60, 70, 290, 400), (20, 30, 100, 120), (25, 40, 110, 111), (0, 64, 200, 201), (5, 6, 7, 7),
              (63, 64, 300, 301), (7, 9, 40, 20), (-9, -2, 0, 301), (0, 64, 301, 400)],
    "everything": [(-1, 65, -1, 302)],
    "one": [(0, 1, 0, 1)],
}


@pytest.mark.parametrize("dtype", [BF, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("batch", [1, 3])
def test_spec_mask_apply_zeroes_the_tables_rectangles_only(dtype, batch):
    from thunder_speech_amd import _lib
    L = _lib.lib()
    ch, t, pitch = 64, 301, 312
    x = (torch.randn(batch, ch, t, generator=torch.Generator().manual_seed(batch)) + 4.0).to(dtype)
    for name, table in MASK_TABLES.items():
        for n_masks in (len(table), 0):
            what = f"spec apply {name} n_masks={n_masks} batch={batch} {dtype}"
            buf, feats = _rows(batch * ch, pitch, dtype)
            f3 = feats.view(batch, ch, pitch)
            f3[:, :, :t] = x.cuda()
            f3[:, :, t:] = PAD
            td = torch.tensor(table, dtype=torch.int32).cuda()
            st = L.ts_spec_mask_apply(feats.data_ptr(), x.element_size(), batch, ch, t, pitch, td.data_ptr() if n_masks else None, n_masks, _stream())
            assert st == 0, what
            torch.cuda.synchronize()
            _rows_ok(buf, batch * ch, what)
            got = f3.cpu()
            assert bool((got[:, :, t:] == PAD).all()), f"{what}: the columns between t and the pitch were written"
            want = mask_reference(x, table[:n_masks])
            _exact("spec-apply", what, _bits(got[:, :, :t]), _bits(want))
            if name == "everything" and n_masks:
                assert bool((got[:, :, :t] == 0).all())
    E = _lib.TS_EINVAL
    a = feats.data_ptr()
    for args in [(None, 4, 1, 64, 301, 312, a, 1), (a, 3, 1, 64, 301, 312, a, 1), (a, 4, 1, 64, 301, 300, a, 1), (a, 4, 1, 64, 301, 312, None, 1),
                 (a, 4, 1, 64, 301, 312, a, -1), (a, 4, 0, 64, 301, 312, a, 1)]:
        assert L.ts_spec_mask_apply(*args, None) == E, args


# ---------------------------------------------------------------------------------------------------------------------
# 9. ts_spec_masks_draw
# ---------------------------------------------------------------------------------------------------------------------
def philox_words(seed, stream_id, counter):
    """Philox4x32-10 (Salmon et al., SC'11) on numpy uint64 arrays: the four 32-bit words of philox(seed, stream, counter)"""
    m32 = np.uint64(0xFFFFFFFF)
    c0, c1 = counter & m32, counter >> np.uint64(32)
    c2, c3 = np.full_like(counter, stream_id), np.zeros_like(counter)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return c0, c1, c2, c3


def spans_reference(u_value, u_min, mask_param, size):
    """float32 arrays of draws -> (start, end, min_value): value = u W and min_value = u' (size - value), every step rounded to float32; long() truncates"""
    value = (u_value * np.float32(mask_param)).astype(np.float32)
    room = (np.float32(size) - value).astype(np.float32)
    min_value = (u_min * room).astype(np.float32)
    start = np.trunc(min_value).astype(np.int64)
    return start, start + np.trunc(value).astype(np.int64), min_value


def draw_reference(seed, n_mels, n_frames, n_time, time_width, n_freq, freq_width, n_cutout, cut_freq_width):
    """-> (table int32 [n][4], min_value of every span): cutout rows use two counters each (frequency span, then a time span with cut_freq_width), then
    the time rows, then the frequency rows, one counter each; draw j is words 0 and 1 of philox(seed, stream 2, j)"""
    n_draws = 2 * n_cutout + n_time + n_freq
    w = philox_words(seed, 2, np.arange(n_draws, dtype=np.uint64))
    u0 = (w[0] >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    u1 = (w[1] >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    c = 2 * n_cutout
    f0, f1, mf = spans_reference(u0[0:c:2], u1[0:c:2], cut_freq_width, n_mels)
    t0, t1, mt = spans_reference(u0[1:c:2], u1[1:c:2], cut_freq_width, n_frames)
    rows = [np.stack([f0, f1, t0, t1], axis=1)]
    t0, t1, m2 = spans_reference(u0[c: c + n_time], u1[c: c + n_time], time_width, n_frames)
    rows.append(np.stack([np.zeros_like(t0), np.full_like(t0, n_mels), t0, t1], axis=1))
    f0, f1, m3 = spans_reference(u0[c + n_time:], u1[c + n_time:], freq_width, n_mels)
    rows.append(np.stack([f0, f1, np.zeros_like(f0), np.full_like(f0, n_frames)], axis=1))
    return np.concatenate(rows).astype(np.int32), np.concatenate([mf, mt, m2, m3])


# the last two were searched for with the restatement alone: forming size - u W with one rounding (a contracted fma) instead of two changes two table
# entries at seed 248 with the typical widths, and at seed 2806 with the typical and with the oversize widths of the (80, 2001) geometry
DRAW_SEEDS = [1, 99, 2 ** 40 + 17, 0xFEDCBA9876543210, 123456789, 248, 2806]
DRAW_GEOMETRIES = [(80, 2001), (64, 1), (1, 7)]
DRAW_ROWS = 2000
NEAR = 1e-3


def draw_widths(n_mels, n_frames):
    """(time_width, freq_width, cut_freq_width) sets: typical, 0 and 1, equal to the size, larger than the size (min_value < 0 truncates toward zero)"""
    return [(100, 27, 33), (0, 1, 1), (1, 0, 0), (n_frames, n_mels, n_mels), (n_frames + 50, n_mels + 30, n_mels + 7), (n_frames, n_mels, n_frames)]


def near_integer_share(min_value):
    return float((np.abs(min_value - np.rint(min_value)) < NEAR).mean())


NEAR_FLOOR = 1e-3                         # half of the 2e-3 that draws spread over many units give (module docstring)


@pytest.mark.parametrize("n_mels,n_frames", DRAW_GEOMETRIES)
def test_spec_masks_draw_matches_the_philox_restatement_over_thousands_of_rows(n_mels, n_frames):
    from thunder_speech_amd import _lib
    L = _lib.lib()
    n = 3 * DRAW_ROWS
    n_bad, near = 0, 0
    for tw, fw, cfw in draw_widths(n_mels, n_frames):
        for seed in DRAW_SEEDS:
            what = f"spec draw seed={seed} mels={n_mels} frames={n_frames} widths=({tw}, {fw}, {cfw})"
            want, min_value = draw_reference(seed, n_mels, n_frames, DRAW_ROWS, tw, DRAW_ROWS, fw, DRAW_ROWS, cfw)
            share = near_integer_share(min_value)
            near += int(round(share * min_value.size))
            buf, table = _flat(4 * n, torch.int32, -7777, -7)
            st = L.ts_spec_masks_draw(seed, DRAW_ROWS, tw, DRAW_ROWS, fw, DRAW_ROWS, 12345, cfw, n_mels, n_frames, table.data_ptr(), _stream())
            assert st == 0, what
            torch.cuda.synchronize()
            _flat_ok(buf, 4 * n, -7, what)
            bad = int((table.cpu().numpy().reshape(n, 4) != want).sum())
            n_bad += bad
            print(f"RATIO|spec-draw|{float(bad):.3e}|{what} near-integer share {share:.2e}")
            assert bad == 0, f"{what}: {bad} table entries differ"
            assert share >= NEAR_FLOOR, f"{what}: only {share:.2e} of the spans have min_value within {NEAR} of an integer"
    assert near > 100
    buf, table = _flat(8, torch.int32, -7777, -7)
    assert L.ts_spec_masks_draw(1, 0, 5, 0, 5, 0, 5, 5, 80, 100, table.data_ptr(), None) == 0            # nothing to draw: no launch
    torch.cuda.synchronize()
    assert bool((table == -7777).all())
    E = _lib.TS_EINVAL
    for args in [(1, 1, 5, 0, 5, 0, 5, 5, 80, 100, None), (1, -1, 5, 0, 5, 0, 5, 5, 80, 100, table.data_ptr()), (1, 1, 5, 0, 5, 0, 5, 5, 0, 100, table.data_ptr()),
                 (1, 1, 5, 0, 5, 0, 5, 5, 80, 0, table.data_ptr())]:
        assert L.ts_spec_masks_draw(*args, None) == E, args
