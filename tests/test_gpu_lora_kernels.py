"""GPU checks of the LoRA launches (csrc/lora_train.hip through include/thunder_speech_amd/lora_train.h, raw C ABI): the forward into the middle slice
of a [rows][3 n] buffer and the backward against a float64 restatement that reads the same bf16 operands and rounds u and g to bf16 where the kernels
do, so what remains is accumulation order.  Bounds: those of tests/test_gpu_mms_adapter_train.py for bf16 operands (the same operand widths and the
same kind of sums over rows), scaled by the reference's max magnitude as there."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SENTINEL = 12345.0
SHAPES = [(1, 128, 128, 8),          # one row of a 16-row tile, rank 8 padded to the k-step
          (37, 128, 128, 16),        # rows % 16 != 0
          (300, 320, 320, 64),       # two k-steps over the rank, three row ranges (100 rows each), k % 64 != 0
          (300, 1280, 1280, 16)]     # the XLS-R 1B width, three row ranges
GRAD_BOUND = 2e-2                    # tests/test_gpu_mms_adapter_train.py: GRAD_BOUND[1], relative to max|reference|
SCALE = 2.0                          # alpha / r


def _out_bound(delta, base):
    """tests/test_gpu_mms_adapter_train.py's output bound in mixed precision: 1 % of the added term's max + 1e-5 of what it is added to."""
    return 0.01 * float(delta.abs().max()) + 1e-5 * float(base.abs().max())


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _bf_round(t64):
    return t64.float().to(BF).double()


def _restate(x, a, b, dy, scale):
    """float64 on the bf16 operands: u and g rounded to bf16 where the kernels round them."""
    xd, ad, bd, dyd = x.double(), a.double(), b.double(), dy.double()
    u = _bf_round(xd @ ad.T)
    delta = scale * (u @ bd.T)
    g = _bf_round(scale * (dyd @ bd))
    return dict(u=u, delta=delta, g=g, dx=g @ ad, d_a=g.T @ xd, d_b=scale * (dyd.T @ u))


def _make(rows, k, n, r, integers=False):
    gen = torch.Generator().manual_seed(rows + 3 * k + 5 * n + 7 * r + int(integers))
    if integers:
        # small integers, exact in bf16 and in every f32 sum: the result must be exactly equal (a swapped lane map cannot hide)
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=gen).float()
        x, a, b, dy = ri(-2, 2, rows, k), ri(-1, 1, r, k), ri(-1, 2, n, r), ri(-2, 1, rows, n)
        base, dx0 = ri(-8, 8, rows, n), ri(-8, 8, rows, k)
    else:
        x, dy = torch.randn(rows, k, generator=gen), torch.randn(rows, n, generator=gen)
        a, b = torch.randn(r, k, generator=gen) / k ** 0.5, torch.randn(n, r, generator=gen) / r ** 0.5
        base, dx0 = torch.randn(rows, n, generator=gen), torch.randn(rows, k, generator=gen)
    x, a, b, dy = x.to(BF), a.to(BF), b.to(BF), dy.to(BF)
    case = dict(x=x, a=a, b=b, dy=dy, base=base, dx0=dx0)
    case.update(_restate(x, a, b, dy, SCALE))
    return case


_CASES = {}


def _case(rows, k, n, r, integers=False):
    key = (rows, k, n, r, integers)
    if key not in _CASES:
        _CASES[key] = _make(*key)
    return _CASES[key]


def _forward(c, rows, k, n, r, b=None):
    """-> (the [rows + 16][3 n] buffer, u16, status): the target is the middle slice; sentinels around it and 16 sentinel rows behind it."""
    from thunder_speech_amd import _lib
    L = _lib.lib()
    y = torch.full((rows + 16, 3 * n), SENTINEL, device="cuda")
    y[:rows, n:2 * n] = c["base"].cuda()
    u16 = torch.full((rows + 16, r), SENTINEL, device="cuda").to(BF)
    x, a = c["x"].cuda(), c["a"].cuda()
    b = (c["b"] if b is None else b).cuda()
    st = L.ts_lora_fwd(x.data_ptr(), rows, k, a.data_ptr(), b.data_ptr(), n, r, SCALE, y.data_ptr() + 4 * n, 3 * n, u16.data_ptr(), _stream())
    torch.cuda.synchronize()
    return y, u16, st


def _backward(c, rows, k, n, r, want_dx=True):
    """-> (dx or None, d_a, d_b, status): dy16 is the middle slice of a [rows][3 n] bf16 copy, d_a / d_b and the workspace poisoned with NaN."""
    from thunder_speech_amd import _lib
    L = _lib.lib()
    dy3 = torch.full((rows, 3 * n), 77.0, device="cuda").to(BF)
    dy3[:, n:2 * n] = c["dy"].cuda()
    x, u16 = c["x"].cuda(), c["u"].to(BF).cuda()
    at16, bt16 = c["a"].T.contiguous().cuda(), c["b"].T.contiguous().cuda()
    dx = None
    if want_dx:
        dx = torch.full((rows + 16, k), SENTINEL, device="cuda")
        dx[:rows] = c["dx0"].cuda()
    d_a, d_b = torch.full((r, k), float("nan"), device="cuda"), torch.full((n, r), float("nan"), device="cuda")
    nbytes = L.ts_lora_bwd_workspace(rows, k, n, r)
    assert nbytes > 0 and nbytes % 4 == 0
    ws = torch.full((nbytes // 4,), float("nan"), device="cuda")
    st = L.ts_lora_bwd(dy3.data_ptr() + 2 * n, 3 * n, x.data_ptr(), u16.data_ptr(), rows, k, n, r, SCALE, at16.data_ptr(), bt16.data_ptr(), _ptr(dx),
                       d_a.data_ptr(), d_b.data_ptr(), ws.data_ptr(), _stream())
    torch.cuda.synchronize()
    return dx, d_a, d_b, st


@pytest.mark.parametrize("rows,k,n,r", SHAPES)
def test_forward_adds_the_low_rank_term_into_the_middle_slice(rows, k, n, r):
    c = _case(rows, k, n, r)
    y, u16, st = _forward(c, rows, k, n, r)
    assert st == 0
    assert bool((y[:, :n] == SENTINEL).all()) and bool((y[:, 2 * n:] == SENTINEL).all()) and bool((y[rows:] == SENTINEL).all())
    assert bool((u16[rows:].float() == torch.tensor(SENTINEL).to(BF).float()).all())
    u_err = float((u16[:rows].double().cpu() - c["u"]).abs().max())
    assert u_err <= 2.0 ** -7 * float(c["u"].abs().max())                       # bf16: at most one unit in the last place of the largest element
    got = y[:rows, n:2 * n].double().cpu()
    ref = c["base"].double() + c["delta"]
    err, bound = float((got - ref).abs().max()), _out_bound(c["delta"], c["base"])
    print(f"lora fwd rows={rows} k={k} n={n} r={r}: y err {err:.3e} (bound {bound:.3e}), u err {u_err:.3e}")
    assert float(c["delta"].abs().max()) > 0.5 * float(c["base"].abs().max())   # the term is not hidden by the base
    assert err <= bound, (err, bound)
    # B = 0: the slice is the base, bit for bit
    y0, _, st = _forward(c, rows, k, n, r, b=torch.zeros_like(c["b"]))
    assert st == 0 and torch.equal(y0[:rows, n:2 * n].cpu(), c["base"])


@pytest.mark.parametrize("rows,k,n,r", SHAPES)
def test_backward_matches_the_float64_restatement(rows, k, n, r):
    from thunder_speech_amd import _lib
    if rows == 300:                                                              # the sums over rows span more than one range here
        one = _lib.lib().ts_lora_bwd_workspace(128, k, n, r) - 4 * 128 * r
        assert _lib.lib().ts_lora_bwd_workspace(rows, k, n, r) - 4 * rows * r == 3 * one
    c = _case(rows, k, n, r)
    dx, d_a, d_b, st = _backward(c, rows, k, n, r)
    assert st == 0 and bool((dx[rows:] == SENTINEL).all())
    got = dict(dx=dx[:rows].double().cpu() - c["dx0"].double(), d_a=d_a.double().cpu(), d_b=d_b.double().cpu())
    errs = {}
    for name, t in got.items():
        assert not bool(torch.isnan(t).any()), f"{name}: unwritten (NaN) elements"
        errs[name] = float((t - c[name]).abs().max()) / float(c[name].abs().max())
    print(f"lora bwd rows={rows} k={k} n={n} r={r}: " + " ".join(f"{m} {e:.2e}" for m, e in errs.items()) + f" (bound {GRAD_BOUND:.0e})")
    for name, e in errs.items():
        assert e <= GRAD_BOUND, (name, e)
    # dx = NULL (no upstream gradient wanted): the two parameter gradients, bit for bit
    none, d_a2, d_b2, st = _backward(c, rows, k, n, r, want_dx=False)
    assert st == 0 and none is None and torch.equal(d_a, d_a2) and torch.equal(d_b, d_b2)


def test_two_runs_give_the_same_bits():
    rows, k, n, r = 300, 1280, 1280, 16
    c = _case(rows, k, n, r)
    y1, u1, _ = _forward(c, rows, k, n, r)
    y2, u2, _ = _forward(c, rows, k, n, r)
    assert torch.equal(y1, y2) and torch.equal(u1.float(), u2.float())
    one, two = _backward(c, rows, k, n, r), _backward(c, rows, k, n, r)
    for t1, t2 in zip(one[:3], two[:3]):
        assert torch.equal(t1, t2) and not bool(torch.isnan(t1).any())


@pytest.mark.parametrize("rows,k,n,r", [(37, 128, 160, 8), (300, 320, 256, 64), (50, 160, 128, 32)])
def test_small_integers_come_out_exactly(rows, k, n, r):
    """x, A, B, dy small asymmetric integers: every product and f32 sum is exact and u, g round the same way in any order, so a wrong lane map, a
    swapped row / column or a lost k-step shows as an unequal element."""
    c = _case(rows, k, n, r, integers=True)
    y, u16, st = _forward(c, rows, k, n, r)
    assert st == 0
    assert torch.equal(u16[:rows].double().cpu(), c["u"])
    assert torch.equal(y[:rows, n:2 * n].double().cpu(), c["base"].double() + c["delta"])
    dx, d_a, d_b, st = _backward(c, rows, k, n, r)
    assert st == 0
    assert torch.equal(dx[:rows].double().cpu(), c["dx0"].double() + c["dx"])
    assert torch.equal(d_a.double().cpu(), c["d_a"]) and torch.equal(d_b.double().cpu(), c["d_b"])


def test_entry_points_refuse_what_they_do_not_take():
    from thunder_speech_amd import _lib
    L = _lib.lib()
    assert L.ts_lora_abi_version() == 1
    rows, k, n, r = 4, 128, 128, 16
    h16 = torch.zeros(rows * 3 * n, device="cuda").to(BF)
    w16 = torch.zeros(64 * 128, device="cuda").to(BF)
    f = torch.zeros(1 << 14, device="cuda")                        # d_a [64][128] is the largest f32 result of the calls below
    ws = torch.zeros(1 << 18, device="cuda")
    EINVAL, EUNSUP = _lib.TS_EINVAL, _lib.TS_EUNSUPPORTED

    def fwd(rr=rows, kk=k, nn=n, rk=r, ld=3 * n, **over):
        p = dict(x16=h16, a16=w16, b16=w16, y=f, u16=h16)
        p.update(over)
        q = {m: (t if isinstance(t, int) else _ptr(t)) for m, t in p.items()}
        return L.ts_lora_fwd(q["x16"], rr, kk, q["a16"], q["b16"], nn, rk, 1.0, q["y"], ld, q["u16"], _stream())

    def bwd(rr=rows, kk=k, nn=n, rk=r, ld=3 * n, **over):
        p = dict(dy16=h16, x16=h16, u16=h16, at16=w16, bt16=w16, dx=f, d_a=f, d_b=f, ws=ws)
        p.update(over)
        q = {m: (t if isinstance(t, int) else _ptr(t)) for m, t in p.items()}
        return L.ts_lora_bwd(q["dy16"], ld, q["x16"], q["u16"], rr, kk, nn, rk, 1.0, q["at16"], q["bt16"], q["dx"], q["d_a"], q["d_b"], q["ws"], _stream())

    assert fwd() == 0 and bwd() == 0 and bwd(dx=None) == 0
    assert all(fwd(rk=v) == 0 and bwd(rk=v) == 0 for v in (8, 16, 32, 64))
    for call, required in ((fwd, ("x16", "a16", "b16", "y", "u16")), (bwd, ("dy16", "x16", "u16", "at16", "bt16", "d_a", "d_b", "ws"))):
        for name in required:
            assert call(**{name: None}) == EINVAL, name
        assert call(rr=0) == EINVAL and call(rr=-1) == EINVAL and call(kk=0) == EINVAL and call(nn=0) == EINVAL and call(rk=0) == EINVAL
        assert call(ld=n - 32) == EINVAL
        assert call(rk=12) == EUNSUP and call(rk=4) == EUNSUP and call(rk=128) == EUNSUP and call(kk=100) == EUNSUP and call(nn=100, ld=400) == EUNSUP
        assert call(ld=3 * n + 2) == EUNSUP
        for name in required + (("dx",) if call is bwd else ()):
            assert call(**{name: f.data_ptr() + 4}) == EUNSUP, name                    # 4-byte aligned only
    W = L.ts_lora_bwd_workspace
    assert W(0, k, n, r) == EINVAL and W(rows, 0, n, r) == EINVAL and W(rows, k, 0, r) == EINVAL and W(rows, k, n, 0) == EINVAL and W(rows, k, n, r) > 0
    torch.cuda.synchronize()
