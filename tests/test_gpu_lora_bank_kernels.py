"""GPU checks of the LoRA bank launch (csrc/lora_bank.hip through include_staged/thunder_speech_amd/queued/lora_bank.h, raw C ABI) in the style of
tests/test_gpu_lora_kernels.py: a float64 restatement on the same operands with u rounded to bf16 where the kernel rounds it, sentinel columns around
the target slices and 16 sentinel rows behind the last clip.

Bounds.
  f32 y, bf16 operands:  |got - (base + delta)| <= e = 0.01 max|delta| + 1e-5 max|base| -- tests/test_gpu_lora_kernels.py::_out_bound, for the same
      operand widths and the same kind of sums.
  bf16 y:  the same e, plus the final rounding to bf16 (half a unit in the last place: 2^-9 relative) of a value within e of the reference:
      e + 2^-9 (|ref| + e) per element against the unrounded float64 ref.
  f32 instantiation, per element of y_i = base_i + s sum_j B_ij u_j, u_j = sum_l A_jl x_l, with unit roundoff w = 2^-24: a dot product of k f32 terms
      has forward error <= k w sum_l |A_jl| |x_l| in any summation order (Higham, Accuracy and Stability of Numerical Algorithms, 3.1; fused
      multiply-adds only lower it), so |u^_j - u_j| <= k w U_j with U_j = sum_l |A_jl| |x_l|; the second dot product over r terms adds
      r w sum_j |B_ij| |u^_j|, the scaling by s one rounding and the final add one rounding of the result.  To first order in w:
      |got_i - ref_i| <= (k + r + 2) w s sum_j |B_ij| U_j + w |ref_i|."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SENTINEL = 12345.0
SCALES = [2.0, 1.5, 0.5, 1.0]                   # alpha / r per slot: all different, exact in binary
W = 2.0 ** -24

# (batch, t, k = n, r, slots, ids); the form (target offsets, in units of n; pitch) comes with each test
S1 = (3, 37, 128, 8, 3, (2, -1, 0))
S2 = (5, 1, 128, 16, 2, (1, 0, 1, -1, 0))
S3 = (2, 16, 320, 64, 2, (1, 1))
S4 = (2, 300, 1280, 16, 4, (0, 3))
MIDDLE, QKV, QV, OUT = "middle", "qkv", "qv", "out"
FORMS = {MIDDLE: ((1,), 3, 0),           # one target in the middle slice of a [rows][3 n] buffer
         QKV: ((0, 1, 2), 3, 16),        # three targets at 0, n, 2 n, and 16 sentinel columns behind them
         QV: ((0, 2), 3, 0),             # q and v at 0 and 2 n: the middle slice keeps its sentinel
         OUT: ((0,), 1, 0)}              # the out_proj form: ldy = n


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bf_round(t64):
    return t64.float().to(BF).double()


def _make(shape, form, x_bf16, y_bf16, integers):
    batch, t, k, r, slots, ids = shape
    n = k
    offs, width, extra = FORMS[form]
    nt, rows, ldy = len(offs), batch * t, width * n + extra
    gen = torch.Generator().manual_seed(batch + 3 * t + 5 * k + 7 * r + 11 * nt + int(integers))
    if integers:
        # small integers, exact in bf16 and in every f32 sum, a different pattern in every slot and target (a generator's stream does not repeat)
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=gen).float()
        x, a, b, base = ri(-2, 2, rows, k), ri(-1, 1, slots, nt, r, k), ri(-1, 2, slots, nt, n, r), ri(-8, 8, rows, nt, n)
    else:
        x, base = torch.randn(rows, k, generator=gen), torch.randn(rows, nt, n, generator=gen)
        a, b = torch.randn(slots, nt, r, k, generator=gen) / k ** 0.5, torch.randn(slots, nt, n, r, generator=gen) / r ** 0.5
    od = BF if x_bf16 else torch.float32
    x, a, b = x.to(od), a.to(od), b.to(od)
    base = base.to(BF if y_bf16 else torch.float32)
    scales = torch.tensor(SCALES[:slots])
    # float64 on the operands as stored
    delta = torch.zeros(rows, nt, n, dtype=torch.float64)
    mag = torch.zeros(rows, nt, n, dtype=torch.float64)               # s sum_j |B_ij| sum_l |A_jl| |x_l|: the f32 instantiation's bound
    for c, slot in enumerate(ids):
        if not 0 <= slot < slots:
            continue
        xc = x[c * t:(c + 1) * t].double()
        for j in range(nt):
            u = xc @ a[slot, j].double().T
            if x_bf16:
                u = _bf_round(u)
            delta[c * t:(c + 1) * t, j] = float(scales[slot]) * (u @ b[slot, j].double().T)
            mag[c * t:(c + 1) * t, j] = float(scales[slot]) * ((xc.abs() @ a[slot, j].double().abs().T) @ b[slot, j].double().abs().T)
    return dict(x=x, a=a, b=b, base=base, scales=scales, delta=delta, mag=mag, ref=base.double() + delta, cols=[o * n for o in offs], ldy=ldy,
                rows=rows, n=n, nt=nt, ids=torch.tensor(ids, dtype=torch.int32))


_CASES = {}


def _case(shape, form, x_bf16=True, y_bf16=True, integers=False):
    key = (shape, form, x_bf16, y_bf16, integers)
    if key not in _CASES:
        _CASES[key] = _make(*key)
    return _CASES[key]


def _run(c, shape, x_bf16, y_bf16, ids=None):
    """-> (the [rows + 16][ldy] buffer as the launch left it, the same buffer before the launch, status)."""
    from thunder_speech_amd import _lib
    batch, t, k, r, slots, _ = shape
    rows, n, nt = c["rows"], c["n"], c["nt"]
    y = torch.full((rows + 16, c["ldy"]), SENTINEL, device="cuda").to(BF if y_bf16 else torch.float32)
    for j, col in enumerate(c["cols"]):
        y[:rows, col:col + n] = c["base"][:, j].cuda()
    before = y.clone()
    x, a, b, scales = c["x"].cuda(), c["a"].cuda(), c["b"].cuda(), c["scales"].cuda()
    ids = (c["ids"] if ids is None else torch.tensor(ids, dtype=torch.int32)).cuda()
    cols = c["cols"] + [-1] * (3 - nt)
    st = _lib.lib().ts_lora_bank_fwd(x.data_ptr(), int(x_bf16), k, batch, t, k, a.data_ptr(), b.data_ptr(), scales.data_ptr(), slots, nt, n, r,
                                     ids.data_ptr(), y.data_ptr(), int(y_bf16), c["ldy"], cols[0], cols[1], cols[2], _stream())
    torch.cuda.synchronize()
    return y, before, st


def _slices(c, y):
    """[rows][nt][n]: the target slices of the buffer."""
    return torch.stack([y[:c["rows"], col:col + c["n"]] for col in c["cols"]], 1)


def _outside_kept(c, y, before):
    """Everything outside the target slices and behind the last row keeps its bits (the sentinel)."""
    mask = torch.ones_like(y, dtype=torch.bool)
    for col in c["cols"]:
        mask[:c["rows"], col:col + c["n"]] = False
    return bool((y.view(torch.int16 if y.dtype == BF else torch.int32)[mask] == before.view(torch.int16 if y.dtype == BF else torch.int32)[mask]).all())


def _adapted_rows(shape):
    batch, t, _, _, slots, ids = shape
    rows = torch.zeros(batch * t, dtype=torch.bool)
    for c, slot in enumerate(ids):
        rows[c * t:(c + 1) * t] = 0 <= slot < slots
    return rows


def _check(shape, form, x_bf16, y_bf16):
    c = _case(shape, form, x_bf16, y_bf16)
    y, before, st = _run(c, shape, x_bf16, y_bf16)
    assert st == 0
    assert _outside_kept(c, y, before)
    got = _slices(c, y).double().cpu()
    on = _adapted_rows(shape)
    assert torch.equal(_slices(c, y).cpu()[~on], c["base"][~on])                 # a clip with id -1: its rows keep their bits
    err = (got - c["ref"]).abs()
    if not x_bf16:
        bound = (shape[2] + shape[3] + 2) * W * c["mag"] + W * c["ref"].abs()
    else:
        e = 0.01 * float(c["delta"].abs().max()) + 1e-5 * float(c["base"].double().abs().max())
        bound = e + 2.0 ** -9 * (c["ref"].abs() + e) if y_bf16 else torch.full_like(err, e)
    worst = float((err - bound).max())
    print(f"lora bank {shape[:5]} {form} x_bf16={x_bf16} y_bf16={y_bf16}: max err {float(err.max()):.3e}, max bound {float(bound.max()):.3e}, "
          f"max (err - bound) {worst:.3e}")
    assert float(c["delta"][on].abs().max()) > 0.5 * float(c["base"].double().abs().max())      # the term is not hidden by the base
    assert bool((err <= bound).all()), worst


@pytest.mark.parametrize("shape,form", [(S1, MIDDLE), (S2, MIDDLE), (S3, QKV), (S4, QV)])
def test_bf16_rows_get_their_clips_term(shape, form):
    _check(shape, form, True, True)


@pytest.mark.parametrize("shape", [S2, S4])
def test_out_proj_form_adds_into_the_f32_residual(shape):
    _check(shape, OUT, True, False)


@pytest.mark.parametrize("shape,form", [(S1, MIDDLE), (S3, QKV)])
def test_f32_instantiation(shape, form):
    _check(shape, form, False, False)


@pytest.mark.parametrize("shape,form,y_bf16", [(S1, MIDDLE, True), (S3, QKV, True), (S4, QV, True), (S4, OUT, False), (S3, QKV, False)])
def test_small_integers_come_out_exactly(shape, form, y_bf16):
    """Every product and f32 sum is exact, u rounds the same way in any order and so does the final bf16 value: a wrong slot, a wrong target, a wrong
    clip boundary or a swapped lane map shows as an unequal element."""
    c = _case(shape, form, True, y_bf16, integers=True)
    y, before, st = _run(c, shape, True, y_bf16)
    assert st == 0 and _outside_kept(c, y, before)
    want = c["ref"].float().to(BF).double() if y_bf16 else c["ref"]
    assert torch.equal(_slices(c, y).double().cpu(), want)
    assert not torch.equal(want[_adapted_rows(shape)], c["base"].double()[_adapted_rows(shape)])


@pytest.mark.parametrize("x_bf16", [True, False])
def test_f32_integers_and_out_of_range_ids_keep_their_rows(x_bf16):
    """Ids -1, n_slots and 2^30 select nothing: the clips' rows keep their bits; the clip with a valid id next to them gets its term, exactly."""
    shape = (4, 37, 128, 8, 3, (-1, 3, 2 ** 30, 1))
    c = _case(shape, QV, x_bf16, x_bf16, integers=True)
    y, before, st = _run(c, shape, x_bf16, x_bf16)
    assert st == 0 and _outside_kept(c, y, before)
    got = _slices(c, y).cpu()
    assert torch.equal(got[:3 * 37], c["base"][:3 * 37])
    want = c["ref"].float().to(BF).double() if x_bf16 else c["ref"]
    assert torch.equal(got.double(), want) and not torch.equal(got[3 * 37:], c["base"][3 * 37:])
    # all clips out of range: the whole buffer keeps its bits
    y, before, st = _run(c, shape, x_bf16, x_bf16, ids=(-1, -2 ** 31, 3, 2 ** 31 - 1))
    assert st == 0 and torch.equal(y.float(), before.float())


def test_two_runs_give_the_same_bits():
    for shape, form, y_bf16 in ((S4, QV, True), (S4, OUT, False), (S3, QKV, True)):
        c = _case(shape, form, True, y_bf16)
        y1, _, _ = _run(c, shape, True, y_bf16)
        y2, _, _ = _run(c, shape, True, y_bf16)
        assert torch.equal(y1.float(), y2.float())
    c = _case(S3, QKV, False, False)
    assert torch.equal(_run(c, S3, False, False)[0], _run(c, S3, False, False)[0])


def test_the_entry_point_refuses_what_it_does_not_take():
    from thunder_speech_amd import _lib
    L = _lib.lib()
    assert L.ts_lora_bank_abi_version() == 1
    EINVAL, EUNSUP = _lib.TS_EINVAL, _lib.TS_EUNSUPPORTED
    batch, t, k, n, r, slots = 2, 4, 128, 128, 16, 2
    x = torch.zeros(batch * t * k, device="cuda").to(BF)
    bank = torch.ones(slots * 3 * 64 * 128, device="cuda").to(BF)
    scales = torch.ones(slots, device="cuda")
    ids = torch.zeros(batch, dtype=torch.int32, device="cuda")
    y = torch.full((batch * t * 3 * n + 64,), SENTINEL, device="cuda")          # f32: large enough for a bf16 or f32 [rows][3 n] (+ slack)
    x32, bank32 = torch.zeros(batch * t * k, device="cuda"), torch.ones(slots * 3 * 64 * 128, device="cuda")

    def call(**over):
        p = dict(x=x.data_ptr(), x_bf16=1, ldx=k, batch=batch, t=t, k=k, a=bank.data_ptr(), b=bank.data_ptr(), scales=scales.data_ptr(), slots=slots,
                 nt=2, n=n, r=r, ids=ids.data_ptr(), y=y.data_ptr(), y_bf16=1, ldy=3 * n, col0=0, col1=2 * n, col2=-1)
        p.update(over)
        return L.ts_lora_bank_fwd(p["x"], p["x_bf16"], p["ldx"], p["batch"], p["t"], p["k"], p["a"], p["b"], p["scales"], p["slots"], p["nt"], p["n"],
                                  p["r"], p["ids"], p["y"], p["y_bf16"], p["ldy"], p["col0"], p["col1"], p["col2"], _stream())

    for name in ("x", "a", "b", "scales", "ids", "y"):
        assert call(**{name: None}) == EINVAL, name
    for name in ("batch", "t", "k", "n", "r", "slots"):
        assert call(**{name: 0}) == EINVAL and call(**{name: -1}) == EINVAL, name
    assert call(nt=0) == EINVAL and call(nt=4) == EINVAL and call(nt=-1) == EINVAL
    assert call(col0=-1) == EINVAL and call(col1=-1) == EINVAL and call(col1=-8) == EINVAL
    assert call(ldx=k - 8) == EINVAL
    assert call(ldy=2 * n) == EINVAL and call(ldy=3 * n - 8) == EINVAL and call(nt=3, col2=3 * n) == EINVAL
    for rank in (4, 12, 24, 128):
        assert call(r=rank) == EUNSUP, rank
    assert call(k=112, ldx=128) == EUNSUP and call(n=112) == EUNSUP
    assert call(batch=65536) == EUNSUP
    assert call(x=x32.data_ptr(), a=bank32.data_ptr(), b=bank32.data_ptr(), x_bf16=0, y_bf16=1) == EUNSUP
    assert call(col1=n - 32) == EUNSUP and call(col1=0) == EUNSUP and call(nt=3, col2=2 * n) == EUNSUP and call(nt=3, col2=n + 64, ldy=4 * n) == EUNSUP
    assert call(ldx=k + 4) == EUNSUP and call(ldy=3 * n + 4) == EUNSUP and call(col1=2 * n + 4, ldy=4 * n) == EUNSUP
    assert call(y_bf16=0, ldy=3 * n + 2) == EUNSUP and call(y_bf16=0, col1=2 * n + 2, ldy=4 * n) == EUNSUP
    for name, t_ in (("x", x), ("a", bank), ("b", bank), ("y", y)):
        assert call(**{name: t_.data_ptr() + 8}) == EUNSUP, name
    assert call(scales=scales.data_ptr() + 2) == EUNSUP and call(ids=ids.data_ptr() + 2) == EUNSUP
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all())                                           # no refusal wrote anything
    # the sizes the refusals were cut from are taken
    for rank in (8, 16, 32, 64):
        assert call(r=rank, nt=3, col1=n, col2=2 * n) == 0
    assert call(x=x32.data_ptr(), a=bank32.data_ptr(), b=bank32.data_ptr(), x_bf16=0, y_bf16=0) == 0
    assert call(nt=1, col1=-1) == 0                                              # offsets of unused targets are ignored
    torch.cuda.synchronize()
