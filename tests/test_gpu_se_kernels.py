"""The eval squeeze-excite kernels (csrc/se.hip) behind ts_se_gate_fwd and ts_se_apply_fwd, launched through the C ABI and compared per element with a
plain float64 restatement on the CPU (sums, einsum, exp in float64; nothing of thunder_speech_amd or oracle), from the operands the device holds:
y and the residual r rounded to bf16 and zero from each clip's length to the pitch, f32 tail constants, f32 weights, int32 lengths.

Restatement:  pool[b, c] = (sum_{e < l} y[b, c, e] + (t - l) tail_y[c]) / t          l = clamp(len[b], 0, t)   (quirk A3: padded frames count)
              h = relu(W1 pool),  s = W2 h,  gate = 1 / (1 + exp(-s))
              out[b, c, e] = act(gate ye + re),  ye = y[e] (e < l) or tail_y[c],  re = r[e r_stride] (e < l) or tail_r[c] (0 without r);
              0 for e >= l with zero_tail, and always 0 for e in [t, pitch_out).

Bound, per element (u32 = 2^-24, u16 = 2^-8; g(n) = n u32 / (1 - n u32); a sum of n rounded products takes every term through at most n roundings
whatever the order of the adds -- lanes, shuffle steps -- so the plain-sum bound g(n) sum |terms| holds for the kernels' lane-strided loops):
  pool   A = sum_{e < l} |y| + (t - l) |tail_y|.  The frame sum has at most t terms; float(t - l) is exact, its product with tail_y, the add and the
         division by t round once each:                              E_pool = g(t + 3) A / t
  fc1    h_j = relu(sum_i w1[j, i] pool[i]), ReLU is 1-Lipschitz:    E_h = |w1| E_pool + g(C) |w1| (|pool| + E_pool)
  fc2                                                                E_s = |w2| E_h + g(hidden) |w2| (|h| + E_h)
  sigmoid through __expf(-s) = v_exp_f32(-s log2 e): log2 e rounded to f32 and the product rounded are two relative errors u32 of the exponent,
         2 u32 |s| log2 e absolute, which exp2 turns into the relative error 2 u32 |s| ln 2 log2 e = 2 u32 |s| (it grows with |s|); v_exp_f32 itself
         is good to 1 ulp = 2 u32.  So e' = exp(-s) (1 + d), |d| <= (2 |s| + 2) u32.  gate = 1 / (1 + e): d gate = -gate (1 - gate) d, and
         gate (1 - gate) <= 1 / 4 also bounds the sigmoid's slope for the incoming E_s.  1 + e rounds once (u32), the reciprocal is v_rcp_f32 under
         -ffast-math (1 ulp = 2 u32):                                E_gate = E_s / 4 + (2 (|s| + E_s) + 2) u32 / 4 + 3 u32 gate
  apply  x = gate ye + re in f32, a product and an add (two roundings; one if contracted to an fma), bf16 operands exact:
                                                                     E_x = E_gate |ye| + u32 (|gate ye| + E_gate |ye|) + u32 (|x| + E_gate |ye|)
         ReLU 1-Lipschitz, then the bf16 store (round to nearest even): E = E_x + u16 (|out| + E_x)
  Frames zeroed by zero_tail and the columns [t, pitch_out) have bound 0: they must be exactly 0.
Nothing here is fitted to measured ratios (profiles/frontend_ctc_se_kernel_checks.md has those).

Conventions as in tests/test_gpu_tcs_kernels.py: the return code is asserted; gate, pool workspace and output sit inside NaN-filled buffers with guard
rows of 7.0 that must come back bit for bit; every check prints `RATIO|kind|error / bound` before it asserts; no element is left out."""
import ctypes as C

import pytest
import torch

NAN = float("nan")
BF = torch.bfloat16
GUARD = 7.0
GUARD_ROWS = 8
U16 = 2.0 ** -8
U32 = 2.0 ** -24


def _g(n):
    return n * U32 / (1 - n * U32)


def _bf(x):
    return x.float().to(BF).float()


def _report(kind, what, err, bound):
    ratio = float((err / bound.clamp_min(1e-300)).max()) if bool((bound > 0).any()) else 0.0
    worst = int((err - bound).argmax())
    print(f"RATIO|{kind}|{ratio:.3e}|{what}")
    assert not bool(torch.isnan(err).any()), f"{what}: unwritten (NaN) elements"
    assert bool((err <= bound).all()), (f"{what}: error {float(err.flatten()[worst]):.3e} > bound {float(bound.flatten()[worst]):.3e} at flat index {worst} "
                                        f"(largest error / bound {ratio:.3e})")
    return ratio


def _operands(b, c, hidden, t, lens, r_stride, pitch_r, seed):
    g = torch.Generator().manual_seed(seed)
    lens_t = torch.tensor(lens)
    l = lens_t.clamp(0, t)
    op = dict(b=b, c=c, hidden=hidden, t=t, lens=lens_t, l=l)
    valid = (torch.arange(t)[None, :] < l[:, None])[:, None, :]
    op["y"] = _bf(torch.randn(b, c, t, generator=g)) * valid
    op["tail_y"] = 0.5 * torch.randn(c, generator=g)
    op["tail_r"] = 0.5 * torch.randn(c, generator=g)
    op["w1"] = torch.randn(hidden, c, generator=g) * (3.0 / c ** 0.5)      # |s| reaches several units: the sigmoid's |s| term matters
    op["w2"] = torch.randn(c, hidden, generator=g) * (3.0 / hidden ** 0.5)
    if r_stride:
        r = torch.zeros(b, c, pitch_r)
        full = _bf(torch.randn(b, c, pitch_r, generator=g))
        for i in range(b):
            n = min(int(l[i]) * r_stride, pitch_r)                        # the residual branch ran at the input's frame rate: l x r_stride valid frames
            r[i, :, :n] = full[i, :, :n]
        op["r"] = r
    return op


def _gate_reference(op):
    """float64 (pool, E_pool, gate, E_gate)"""
    y, t, l = op["y"].double(), op["t"], op["l"].double()
    ty = op["tail_y"].double()[None, :]
    pad = (t - l)[:, None]
    pool = (y.sum(-1) + pad * ty) / t
    a = y.abs().sum(-1) + pad * ty.abs()
    e_pool = _g(t + 3) * a / t
    w1, w2 = op["w1"].double(), op["w2"].double()
    h = torch.relu(pool @ w1.T)
    e_h = e_pool @ w1.abs().T + _g(op["c"]) * ((pool.abs() + e_pool) @ w1.abs().T)
    s = h @ w2.T
    e_s = e_h @ w2.abs().T + _g(op["hidden"]) * ((h.abs() + e_h) @ w2.abs().T)
    gate = 1.0 / (1.0 + torch.exp(-s))
    e_gate = e_s / 4 + (2 * (s.abs() + e_s) + 2) * U32 / 4 + 3 * U32 * gate
    return pool, e_pool, gate, e_gate, s


def _apply_reference(op, gate, e_gate, r_stride, relu, zero_tail):
    """float64 (out, bound) over [b][c][t]; gate / e_gate [b][c] (e_gate 0: the gate handed to the kernel is the reference's own operand)"""
    y, t = op["y"].double(), op["t"]
    valid = (torch.arange(t)[None, :] < op["l"][:, None])[:, None, :]
    ye = torch.where(valid, y, op["tail_y"].double()[None, :, None].expand_as(y))
    if r_stride:
        rs = op["r"].double()[:, :, ::r_stride][:, :, :t]
        assert rs.shape[-1] == t
        re = torch.where(valid, rs, op["tail_r"].double()[None, :, None].expand_as(y))
    else:
        re = torch.zeros_like(y)
    gt, eg = gate[:, :, None], e_gate[:, :, None]
    x = gt * ye + re
    e_x = eg * ye.abs() + U32 * ((gt * ye).abs() + eg * ye.abs()) + U32 * (x.abs() + eg * ye.abs())
    out = torch.relu(x) if relu else x
    bound = e_x + U16 * (out.abs() + e_x)
    if zero_tail:
        out, bound = out * valid, bound * valid
    return out, bound


def _guarded(rows, cols, dtype):
    buf = torch.full((rows + 2 * GUARD_ROWS, cols), NAN, dtype=dtype, device="cuda")
    buf[:GUARD_ROWS] = GUARD
    buf[GUARD_ROWS + rows:] = GUARD
    return buf, buf[GUARD_ROWS: GUARD_ROWS + rows]


def _guards_ok(buf, rows, what):
    g = torch.cat([buf[:GUARD_ROWS], buf[GUARD_ROWS + rows:]])
    assert bool((g == GUARD).all()), f"{what}: a guard row next to the output was written"


def _rows_dev(x, pitch):
    """f32 [b][c][n] (already bf16 values, zero tails) -> bf16 [b][c][pitch] on the device, zero up to the pitch"""
    b, c, n = x.shape
    d = torch.zeros(b, c, pitch, dtype=BF, device="cuda")
    d[:, :, :min(n, pitch)] = x[:, :, :pitch].to(BF).cuda()
    return d


def _stream():
    return torch.cuda.current_stream().cuda_stream


GATE_CASES = [      # channels, hidden, t, pitch, lens
    (20, 3, 70, 72, [70, 33, 0]),
    (20, 8, 70, 72, [70, 33, 0]),
    (20, 3, 513, 520, [513, 33, 0]),        # a second trip of the pooling loop (64 lanes x 8 frames per trip)
    (20, 8, 513, 640, [513, 512, 1]),
]


@pytest.mark.gpu
@pytest.mark.parametrize("c,hidden,t,pitch,lens", GATE_CASES, ids=[f"c{c}-h{h}-t{t}-p{p}" for c, h, t, p, _ in GATE_CASES])
def test_se_gate_matches_the_float64_restatement(c, hidden, t, pitch, lens):
    from thunder_speech_amd import _lib
    L = _lib.lib()
    b = len(lens)
    op = _operands(b, c, hidden, t, lens, 0, 0, seed=t + hidden)
    yd = _rows_dev(op["y"], pitch)
    ld = op["lens"].to(torch.int32).cuda()
    ty, w1, w2 = op["tail_y"].cuda(), op["w1"].cuda(), op["w2"].cuda()
    ws_buf, ws = _guarded(1, b * (c + hidden), torch.float32)
    g_buf, gd = _guarded(b, c, torch.float32)
    st = L.ts_se_gate_fwd(yd.data_ptr(), ld.data_ptr(), ty.data_ptr(), b, c, t, pitch, hidden, w1.data_ptr(), w2.data_ptr(), ws.data_ptr(),
                          gd.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert st == 0
    pool, e_pool, gate, e_gate, s = _gate_reference(op)
    what = f"se gate c={c} hidden={hidden} t={t}"
    _report("se-pool", what, (ws[0, : b * c].view(b, c).double().cpu() - pool).abs(), e_pool)
    _report("se-gate", what, (gd.double().cpu() - gate).abs(), e_gate)
    _guards_ok(ws_buf, 1, what)
    _guards_ok(g_buf, b, what)
    assert float(s.abs().max()) > 1.0 and float(gate.min()) < 0.3 and float(gate.max()) > 0.6      # the inputs exercise the sigmoid away from 1 / 2


def _apply_cases():
    cases = []
    for t, pitch_y in ((70, 72), (513, 520)):
        # residual variants: (r_stride, pitch_r).  Stride 2: the vector path runs while 2 g + 16 <= pitch_r; with pitch_r = 2 x round_up(t, 8) it runs for
        # every group below t, with the smallest legal pitch (round_up(2 (t - 1) + 1, 8)) the last group of a row takes the element-wise fallback
        r8 = (t + 7) // 8 * 8
        small2 = (2 * (t - 1) + 1 + 7) // 8 * 8
        variants = [("nores", 0, 0), ("s1", 1, pitch_y), ("s2-vector", 2, 2 * r8), ("s3", 3, (3 * (t - 1) + 1 + 7) // 8 * 8)]
        if small2 < 2 * r8:                                               # t = 70: the smallest legal pitch already lets the vector path run everywhere
            variants.append(("s2-fallback", 2, small2))
        for name, rs, pr in variants:
            for relu, zt in ((1, 1), (0, 0)) if name in ("s1", "s2-vector") else ((1, 0), (0, 1)):
                cases.append(pytest.param(t, pitch_y, rs, pr, relu, zt, id=f"t{t}-{name}-relu{relu}-zt{zt}"))
    # t = 513 leaves one valid frame (j = 0, where the stride does not enter the index) in the group on the fallback; t = 516 at the same residual
    # pitch 1032 leaves four
    for relu, zt in ((1, 0), (0, 1)):
        cases.append(pytest.param(516, 520, 2, 1032, relu, zt, id=f"t516-s2-fallback-relu{relu}-zt{zt}"))
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("t,pitch_y,r_stride,pitch_r,relu,zero_tail", _apply_cases())
def test_se_apply_matches_the_float64_restatement(t, pitch_y, r_stride, pitch_r, relu, zero_tail):
    """The gate is an operand here (the f32 values the kernel reads), so the apply kernel's own roundings are what is bounded; pitch_out exceeds
    pitch_y by 16 columns, so the groups at and beyond pitch_y (which must not read y) are stored too."""
    from thunder_speech_amd import _lib
    L = _lib.lib()
    c, lens = 20, [t, 33, 0]
    b = len(lens)
    op = _operands(b, c, 3, t, lens, r_stride, pitch_r, seed=3 * t + r_stride)
    if r_stride == 2:
        last = (t - 1) // 8 * 8                                            # first frame of the last group below t
        vector_everywhere = 2 * last + 16 <= pitch_r
        assert vector_everywhere == (pitch_r == 2 * ((t + 7) // 8 * 8)) and 2 * (last - 8) + 16 <= pitch_r
    gate = torch.sigmoid(2.0 * torch.randn(b, c, generator=torch.Generator().manual_seed(t)))
    pitch_out = pitch_y + 16
    yd = _rows_dev(op["y"], pitch_y)
    rd = _rows_dev(op["r"], pitch_r) if r_stride else None
    ld = op["lens"].to(torch.int32).cuda()
    ty, tr, gd = op["tail_y"].cuda(), op["tail_r"].cuda(), gate.cuda()
    buf, out = _guarded(b * c, pitch_out, BF)
    st = L.ts_se_apply_fwd(yd.data_ptr(), rd.data_ptr() if r_stride else None, gd.data_ptr(), ld.data_ptr(), ty.data_ptr(),
                           tr.data_ptr() if r_stride else None, b, c, t, pitch_y, pitch_r, max(r_stride, 1), pitch_out, relu, zero_tail, out.data_ptr(),
                           _stream())
    torch.cuda.synchronize()
    assert st == 0
    ref, bound = _apply_reference(op, gate.double(), torch.zeros(b, c, dtype=torch.float64), r_stride, relu, zero_tail)
    got = out.view(b, c, pitch_out).double().cpu()
    what = f"se apply t={t} r_stride={r_stride} pitch_r={pitch_r} relu={relu} zero_tail={zero_tail}"
    _report("se-apply", what, (got[:, :, :t] - ref).abs(), bound)
    assert bool((got[:, :, t:] == 0).all()), f"{what}: columns [t, pitch_out) are not exactly 0"
    if zero_tail:
        for i, n in enumerate(op["l"].tolist()):
            assert bool((got[i, :, n:] == 0).all()), f"{what}: clip {i} is not exactly 0 from frame {n} on"
    else:
        assert float(ref[1, :, 33:].abs().max()) > 0                       # the reference's constants beyond the length are there
    _guards_ok(buf, b * c, what)
    assert float(ref.abs().max()) > 0.5


@pytest.mark.gpu
def test_se_gate_then_apply_end_to_end():
    """Both entry points chained as a Citrinet block tail chains them: the gate's error E_gate enters the apply bound."""
    from thunder_speech_amd import _lib
    L = _lib.lib()
    b, c, hidden, t, pitch = 3, 20, 8, 70, 72
    op = _operands(b, c, hidden, t, [70, 33, 0], 1, pitch, seed=5)
    yd, rd = _rows_dev(op["y"], pitch), _rows_dev(op["r"], pitch)
    ld = op["lens"].to(torch.int32).cuda()
    ty, tr, w1, w2 = op["tail_y"].cuda(), op["tail_r"].cuda(), op["w1"].cuda(), op["w2"].cuda()
    ws = torch.full((b * (c + hidden),), NAN, device="cuda")
    gd = torch.full((b, c), NAN, device="cuda")
    buf, out = _guarded(b * c, pitch, BF)
    assert L.ts_se_gate_fwd(yd.data_ptr(), ld.data_ptr(), ty.data_ptr(), b, c, t, pitch, hidden, w1.data_ptr(), w2.data_ptr(), ws.data_ptr(),
                            gd.data_ptr(), _stream()) == 0
    assert L.ts_se_apply_fwd(yd.data_ptr(), rd.data_ptr(), gd.data_ptr(), ld.data_ptr(), ty.data_ptr(), tr.data_ptr(), b, c, t, pitch, pitch, 1, pitch,
                             1, 0, out.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    _, _, gate, e_gate, _ = _gate_reference(op)
    ref, bound = _apply_reference(op, gate, e_gate, 1, 1, 0)
    got = out.view(b, c, pitch).double().cpu()
    _report("se-chain", "gate -> apply", (got[:, :, :t] - ref).abs(), bound)
    assert bool((got[:, :, t:] == 0).all())
    _guards_ok(buf, b * c, "gate -> apply")


@pytest.mark.gpu
def test_se_entry_points_refuse_what_they_document():
    """Every TS_EINVAL of the two launchers, on live buffers (the refused calls launch nothing)."""
    from thunder_speech_amd import _lib
    L = _lib.lib()
    E = _lib.TS_EINVAL
    a = torch.zeros(4096, device="cuda").data_ptr()
    gate = dict(y=a, len=a, tail_y=a, batch=2, channels=4, t=16, pitch=16, hidden=2, w1=a, w2=a, pool_ws=a, gate=a)
    order = ["y", "len", "tail_y", "batch", "channels", "t", "pitch", "hidden", "w1", "w2", "pool_ws", "gate"]
    bad = [dict(y=None), dict(len=None), dict(tail_y=None), dict(w1=None), dict(w2=None), dict(pool_ws=None), dict(gate=None), dict(batch=0),
           dict(channels=0), dict(hidden=0), dict(t=0), dict(pitch=8), dict(pitch=20)]
    for ch in bad:
        kw = dict(gate, **ch)
        assert L.ts_se_gate_fwd(*[kw[k] for k in order], None) == E, ch
    apply_ = dict(y=a, r=a, gate=a, len=a, tail_y=a, tail_r=a, batch=2, channels=4, t=16, pitch_y=16, pitch_r=16, r_stride=1, pitch_out=16, relu=1,
                  zero_tail=1, out=a)
    order = ["y", "r", "gate", "len", "tail_y", "tail_r", "batch", "channels", "t", "pitch_y", "pitch_r", "r_stride", "pitch_out", "relu", "zero_tail", "out"]
    bad = [dict(y=None), dict(gate=None), dict(len=None), dict(tail_y=None), dict(out=None), dict(tail_r=None), dict(batch=0), dict(channels=0), dict(t=0),
           dict(pitch_y=8), dict(pitch_out=8), dict(pitch_y=20), dict(pitch_out=20), dict(r_stride=0), dict(pitch_r=8), dict(pitch_r=20),
           dict(r_stride=2, pitch_r=24), dict(r_stride=3, pitch_r=40)]
    for ch in bad:
        kw = dict(apply_, **ch)
        assert L.ts_se_apply_fwd(*[kw[k] for k in order], None) == E, ch
    # without a residual its pitch, stride and tail are not looked at
    kw = dict(apply_, r=None, tail_r=None, r_stride=0, pitch_r=3)
    assert L.ts_se_apply_fwd(*[kw[k] for k in order], None) == 0
    torch.cuda.synchronize()
