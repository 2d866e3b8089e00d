"""The optimizer step, audio preparation and decoder gradient kernels (csrc/train.hip, csrc/dataprep.hip), each called by name through the C ABI with
raw pointers and compared per element with a float64 restatement written here, inside a bound counted from the kernel's code.  Second half of
tests/test_gpu_data_text_optim_kernels.py (the exact checks and the conventions are there); tests/test_data_text_optim_restatements_host.py pins
the restatements on a machine without a GPU.  Nothing of thunder_speech_amd or oracle takes part in the arithmetic; the resampling table that
data/dataset.py builds is read as data.

Entry point             kind of check   restatement
  ts_adamw_step         bounded         torch.optim.AdamW's update in float64 from the f32 operands and the f32-rounded hyper-parameters
  ts_adamw_multi_step   bounded         the same per tensor; bf16 shadow bit-equal to the rounding of the device's own new parameter
  ts_audio_prep         bounded         channel mean, minus the clip mean, torchaudio 0.12 polyphase sinc resampling, in float64
  ts_decoder_bwd        bounded         dW = einsum("bvt,bct->vc"), db = sum over (b, t), in float64 from the same bf16 x and f32 g

Bounds.  u = 2^-24 is the unit roundoff of float32, g(k) = k u / (1 - k u) bounds k roundings in sequence, eta = 2^-126 is added where a product may
fall below the normal range (whether it is then kept as a denormal or flushed).  The library is built with -ffast-math: a / b is a * rcp(b) with
v_rcp_f32 (1 ulp = 2 u) and a product (u), sqrtf is v_sqrt_f32 (1 ulp = 2 u), products feeding sums may or may not be contracted into fused
multiply-adds (the counts below take the unfused, larger figure).  Nothing is fitted to measured ratios (profiles/data_text_optim_kernel_checks.md
has those).

AdamW, per element (p, grad, m, v: the f32 operands; lr, b1, b2, eps, wd: the f32 values the entry point receives; s = step):
  m' = b1 m + (1 - b1) grad       b1 m (u); 1 - b1 (u), times grad (u); the sum (u):         dm = g(1) |b1 m| + g(2) |(1 - b1) grad| + g(1) |m'| + eta
  v' = b2 v + (1 - b2) grad^2     b2 v (u); 1 - b2 (u), two products (2 u); the sum (u):     dv = g(1) |b2 v| + g(3) (1 - b2) grad^2 + g(1) v' + 2 eta
  r = sqrt(v')                    of the perturbed argument, then v_sqrt_f32:                dr = min(dv / r, sqrt(dv)) + g(2) (r + that)
  c_i = 1 - b_i^s                 the host's powf (1 ulp = 2 u) and the subtraction (u):     dc_i = g(2) b_i^s + g(1) c_i,  rc_i = dc_i / c_i
                                  (the restatement forms b_i^s in float64 from the f32 b_i; rc_i <= 1 / 4 is asserted)
  Q = r / sqrt(c2)                sqrtf(c2): relative rc2 / (2 (1 - rc2)) + 2 u; the quotient as rcp and product, or as a product with
                                  1 / sqrtf(c2) formed once (ts_adamw_multi_step): 3 u either way:
                                                                                               dQ = dr / sqrt(c2) (1 + rq) + Q rq,  rq = rc2 / (2 (1 - rc2)) + g(5)
  D = Q + eps                     one sum:                                                     dD = dQ + g(1) (D + dQ)
  a = lr / c1                     relative rc1 / (1 - rc1) + 3 u
  U = a m' / D                    a product (u) and a quotient (3 u) of perturbed operands, dD / D <= 1 / 2 asserted:
                                                                                               dU = (a / D) dm (1 + ra) + |U| (ra + dD / (D - dD)),  ra = rc1 / (1 - rc1) + g(7)
  p1 = p (1 - lr wd)              lr wd (u), the subtraction (u), the product (u):             dp1 = |p| (g(1) |lr wd| + g(1) |1 - lr wd|) + g(1) |p1|
  p' = p1 - U                     one difference:                                              dp = dp1 + dU + g(1) (|p'| + dp1 + dU)
  The two kernels are written differently (sqrtf(v) / sqrtf(c2) against sqrtf(v) * (1 / sqrtf(c2))): their results are compared with the same float64
  bound, not with each other.  The bound on p is dU, relative to the update, plus the roundings of p itself (u |p|, which no f32 result can avoid); the
  operands have |p| from 1e-3 to 1 so that those do not hide the update.  The largest relative term of dU is rq at step 1 with b2 = 0.999: c2 = 1e-3
  is a difference of numbers near 1, rc2 = 2000 u, rq = 6e-5.  Every case prints the medians of dU / |U| and dp / |U| and asserts the first below 1e-4:
  a bias correction that is off by 1e-4 of the step cannot pass.  The first and second moments are checked against dm and dv.
Deviation from torch.optim.AdamW in float64 with double hyper-parameters: the entry points take lr, betas, eps and wd as f32, so the device steps with
  hyper-parameters that are off by up to 2^-24 relative; for b2 = 0.999, 1 - b2 is off by 1.3e-5 relative.  The derived value is the difference of the
  restatement evaluated at the f32-rounded and at the double hyper-parameters; measured <= derived + dp is asserted (profiles/ has the figures).

Audio preparation, per output sample (C channels, t samples, kernel table k[p][j] of kw taps, f32):
  mono = sum_c a_c / C            C - 1 sums, a quotient by rcp and product (3 u):              d_mono = g(C + 2) sum_c |a_c| / C          (0 for C = 1)
  mean                            float64 partial sums of the f32 mono (t terms, 2^-53 each), rounded to f32 once:
                                                                                               d_mean = mean(d_mono) + t 2^-53 mean|mono| + u |mean|
  x = mono - mean                 one difference:                                              d_x = d_mono + d_mean + g(1) (|x| + d_mono + d_mean)
  out = sum_j k_j x_j             kw fused multiply-adds:                                      d_out = sum_j |k_j| d_x_j + g(kw) sum_j |k_j| (|x_j| + d_x_j)
  without resampling out = x and d_out = d_x.  A clip of exact zeros has bound 0 everywhere.

Decoder gradient, per element of dW (and of db with x = 1): the entry point adds one partial per (channel tile, clip group) with atomics; a partial is
  an f32 sum of up to t b products in any order, and up to b partials meet in one element: t b + b roundings at most on any path from a product to
  the result, each product rounded once:                                                    d = g(t b + b + 1) sum_{b, t} |g x|
  Two runs differ by at most 2 d (the atomics' order)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

NAN = float("nan")
BF = torch.bfloat16
GUARD = 7.0
PAD = 9.0
G = 64
U = 2.0 ** -24
ETA = 2.0 ** -126
F64 = torch.float64


def gam(k):
    return k * U / (1.0 - k * U)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _report(kind, what, err, bound):
    ratio = float((err / bound.clamp_min(1e-300)).max()) if bool((bound > 0).any()) else 0.0
    worst = int((err - bound).argmax())
    print(f"RATIO|{kind}|{ratio:.3e}|{what}")
    assert not bool(torch.isnan(err).any()), f"{what}: unwritten (NaN) elements"
    assert bool((err <= bound).all()), (f"{what}: error {float(err.flatten()[worst]):.3e} > bound {float(bound.flatten()[worst]):.3e} at flat index {worst} "
                                        f"(largest error / bound {ratio:.3e})")
    return ratio


def _flat(n, dtype, fill, guard):
    buf = torch.full((n + 2 * G,), fill, dtype=dtype, device="cuda")
    buf[:G] = guard
    buf[G + n:] = guard
    return buf, buf[G: G + n]


def _flat_ok(buf, n, guard, what):
    assert bool((buf[:G] == guard).all()) and bool((buf[G + n:] == guard).all()), f"{what}: a guard element next to the output was written"


def f32(x):
    return float(np.float32(x))


# ---------------------------------------------------------------------------------------------------------------------
# 10. AdamW
# ---------------------------------------------------------------------------------------------------------------------
def adamw_restate(p, grad, m, v, lr, b1, b2, eps, wd, step, bound=True):
    """float64 tensors and Python floats (the values the arithmetic really uses) -> dict p, m, v (+ dp, dm, dv, upd when bound)"""
    c1, c2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    m1 = b1 * m + (1.0 - b1) * grad
    v1 = b2 * v + (1.0 - b2) * grad * grad
    r = v1.sqrt()
    q = r / math.sqrt(c2)
    d = q + eps
    a = lr / c1
    upd = a * m1 / d
    p1 = p * (1.0 - lr * wd)
    out = dict(p=p1 - upd, m=m1, v=v1, upd=upd)
    if not bound:
        return out
    dm = gam(1) * (b1 * m).abs() + gam(2) * ((1.0 - b1) * grad).abs() + gam(1) * m1.abs() + ETA
    dv = gam(1) * (b2 * v).abs() + gam(3) * (1.0 - b2) * grad * grad + gam(1) * v1 + 2 * ETA
    dr = torch.minimum(dv / r.clamp_min(1e-300), dv.sqrt())
    dr = dr + gam(2) * (r + dr)
    rc1 = (gam(2) * b1 ** step + gam(1) * c1) / c1
    rc2 = (gam(2) * b2 ** step + gam(1) * c2) / c2
    assert rc1 <= 0.25 and rc2 <= 0.25
    rq = rc2 / (2.0 * (1.0 - rc2)) + gam(5)
    dq = dr / math.sqrt(c2) * (1.0 + rq) + q * rq
    dd = dq + gam(1) * (d + dq)
    assert bool((dd <= 0.5 * d).all())
    ra = rc1 / (1.0 - rc1) + gam(7)
    du = (a / d) * dm * (1.0 + ra) + upd.abs() * (ra + dd / (d - dd))
    dp1 = p.abs() * (gam(1) * abs(lr * wd) + gam(1) * abs(1.0 - lr * wd)) + gam(1) * p1.abs()
    dp = dp1 + du + gam(1) * (out["p"].abs() + dp1 + du)
    out.update(dp=dp, dm=dm, dv=dv, du=du)
    return out


def adamw_operands(n, seed):
    """f32 p (magnitudes from 1e-3 to 1, so that the update is not lost in the parameter's own rounding), grad with exact zeros, 1e-20 and 1e4, m, v >= 0
    as in the middle of training, with zeros"""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g) * torch.pow(10.0, -3.0 * torch.rand(n, generator=g))
    grad = torch.randn(n, generator=g) * 0.1
    m = torch.randn(n, generator=g) * 0.05
    v = torch.rand(n, generator=g) * 0.01
    idx = torch.arange(n)
    grad[idx % 7 == 0] = 0.0
    grad[idx % 11 == 3] = 1e-20
    grad[idx % 13 == 5] = 1e4
    grad[idx % 17 == 6] = -1e4
    m[idx % 5 == 1] = 0.0
    v[idx % 5 == 1] = 0.0
    v[idx % 19 == 2] = 0.0
    return p, grad, m, v


ADAMW_HYPER = [(lr, betas, eps, wd) for lr in (3e-3,) for betas in ((0.9, 0.999), (0.9, 0.98), (0.0, 0.0)) for eps in (1e-8, 1e-3) for wd in (0.0, 0.05)]
ADAMW_STEPS = [1, 2, 10, 1000, 100000]


def _check_adamw(kind, what, got, ops, hyper, step, ratios):
    p, grad, m, v = ops
    lr, (b1, b2), eps, wd = hyper
    r = adamw_restate(p.double(), grad.double(), m.double(), v.double(), f32(lr), f32(b1), f32(b2), f32(eps), f32(wd), step)
    for name, key in (("p", "dp"), ("m", "dm"), ("v", "dv")):
        ratios[name] = max(ratios.get(name, 0.0), _report(f"{kind}-{name}", what, (got[name].double() - r[name]).abs(), r[key]))
    moving = r["upd"].abs() > 0
    if bool(moving.any()):
        rel = float((r["du"][moving] / r["upd"][moving].abs()).median())
        ratios["dU/|U|"] = max(ratios.get("dU/|U|", 0.0), rel)
        ratios["dp/|U|"] = max(ratios.get("dp/|U|", 0.0), float((r["dp"][moving] / r["upd"][moving].abs()).median()))
        assert rel < 1e-4, f"{what}: the bound on the update is {rel:.2e} of the update in the median"
    return r


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1023, 1025, 29696 + 3])
def test_adamw_step_matches_the_float64_restatement(n):
    from thunder_speech_amd import _lib
    L = _lib.lib()
    ops = adamw_operands(n, n)
    gd = ops[1].cuda()
    ratios = {}
    for hyper in ADAMW_HYPER:
        lr, (b1, b2), eps, wd = hyper
        for step in ADAMW_STEPS:
            what = f"adamw n={n} step={step} betas=({b1}, {b2}) eps={eps} wd={wd}"
            bufs = {}
            for name, src in (("p", ops[0]), ("m", ops[2]), ("v", ops[3])):
                bufs[name] = _flat(n, torch.float32, NAN, GUARD)
                bufs[name][1].copy_(src.cuda())
            st = L.ts_adamw_step(bufs["p"][1].data_ptr(), gd.data_ptr(), bufs["m"][1].data_ptr(), bufs["v"][1].data_ptr(), n, lr, b1, b2, eps, wd, step, _stream())
            assert st == 0, what
            torch.cuda.synchronize()
            for name in bufs:
                _flat_ok(bufs[name][0], n, GUARD, what + " " + name)
            _check_adamw("adamw", what, {k: b[1].cpu() for k, b in bufs.items()}, ops, hyper, step, ratios)
    print(f"RATIO|adamw-summary|n={n}|" + "|".join(f"{k}={v:.3e}" for k, v in ratios.items()))
    assert torch.equal(gd.cpu(), ops[1])


def test_adamw_step_refuses_what_it_documents():
    from thunder_speech_amd import _lib
    L, E = _lib.lib(), _lib.TS_EINVAL
    a = torch.zeros(64, device="cuda").data_ptr()
    for args in [(None, a, a, a, 4), (a, None, a, a, 4), (a, a, None, a, 4), (a, a, a, None, 4), (a, a, a, a, 0)]:
        assert L.ts_adamw_step(*args, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None) == E
    assert L.ts_adamw_step(a, a, a, a, 4, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, None) == E


MULTI_SIZES = [1, 5, 1023, 1024, 1025, 4097, 3 * 1024, 70001, 70001]


def _multi_layout():
    """every tensor's slot in one flat buffer: G guard elements, n elements, and the gap up to the next multiple of 64"""
    offs, pos = [], 0
    for n in MULTI_SIZES:
        offs.append(pos + G)
        pos += G + (n + 63) // 64 * 64
    return offs, pos + G


@pytest.mark.parametrize("hyper,step", [((3e-3, (0.9, 0.999), 1e-8, 0.05), 1), ((3e-3, (0.9, 0.999), 1e-8, 0.05), 1000), ((1e-3, (0.9, 0.98), 1e-3, 0.0), 10),
                                        ((3e-3, (0.0, 0.0), 1e-8, 0.05), 2)])
def test_adamw_multi_step_matches_the_float64_restatement_and_refreshes_the_shadows(hyper, step):
    from thunder_speech_amd import _lib
    L = _lib.lib()
    lr, (b1, b2), eps, wd = hyper
    offs, total = _multi_layout()
    ops = [adamw_operands(n, 100 + i) for i, n in enumerate(MULTI_SIZES)]
    flat = {k: torch.full((total,), GUARD, device="cuda") for k in "pgmv"}
    shadow = torch.full((total,), GUARD, dtype=BF, device="cuda")
    rows = []
    for i, (n, off) in enumerate(zip(MULTI_SIZES, offs)):
        for k, src in zip("pgmv", ops[i]):
            flat[k][off: off + n] = src.cuda()
        has_shadow = i % 2 == 0
        if has_shadow:
            shadow[off: off + n] = NAN
        rows.append([flat["p"][off:].data_ptr(), flat["g"][off:].data_ptr(), flat["m"][off:].data_ptr(), flat["v"][off:].data_ptr(), n,
                     shadow[off:].data_ptr() if has_shadow else 0])
    before = {k: t.cpu() for k, t in flat.items()}
    table = torch.tensor(rows, dtype=torch.int64).cuda()
    what = f"adamw multi step={step} betas=({b1}, {b2}) eps={eps} wd={wd}"
    assert L.ts_adamw_multi_step(table.data_ptr(), len(rows), max(MULTI_SIZES), lr, b1, b2, eps, wd, step, _stream()) == 0, what
    torch.cuda.synchronize()
    after = {k: t.cpu() for k, t in flat.items()}
    sh = shadow.cpu()
    inside = torch.zeros(total, dtype=torch.bool)
    ratios = {}
    for i, (n, off) in enumerate(zip(MULTI_SIZES, offs)):
        inside[off: off + n] = True
        got = {name: after[k][off: off + n] for name, k in (("p", "p"), ("m", "m"), ("v", "v"))}
        _check_adamw("adamw-multi", f"{what} tensor {i} n={n}", got, ops[i], hyper, step, ratios)
        if i % 2 == 0:
            want = got["p"].to(BF)
            bad = int((sh[off: off + n].view(torch.int16) != want.view(torch.int16)).sum())
            print(f"RATIO|adamw-multi-shadow|{float(bad):.3e}|{what} tensor {i} n={n}")
            assert bad == 0, f"{what} tensor {i}: {bad} shadow elements are not the bf16 rounding of the new parameter"
    print("RATIO|adamw-multi-summary|" + "|".join(f"{k}={v:.3e}" for k, v in ratios.items()))
    # everything outside the tensors' own elements: the guards, the elements behind each n, the slots of the tensors without a shadow
    for k in "pmv":
        assert torch.equal(after[k][~inside], before[k][~inside]), f"{what}: {k} was written outside a tensor"
    assert torch.equal(after["g"], before["g"])
    written = torch.zeros(total, dtype=torch.bool)
    for i, (n, off) in enumerate(zip(MULTI_SIZES, offs)):
        if i % 2 == 0:
            written[off: off + n] = True
    assert bool((sh[~written] == GUARD).all()), f"{what}: shadow memory of a tensor without a shadow, or behind a tensor's end, was written"


def test_adamw_multi_step_refuses_what_it_documents():
    from thunder_speech_amd import _lib
    L = _lib.lib()
    a = torch.zeros(64, dtype=torch.int64, device="cuda").data_ptr()
    h = (1e-3, 0.9, 0.999, 1e-8, 0.0)
    assert L.ts_adamw_multi_step(a, 65536, 4, *h, 1, None) == _lib.TS_EUNSUPPORTED
    assert L.ts_adamw_multi_step(a, 1, 4, *h, 0, None) == _lib.TS_EINVAL and L.ts_adamw_multi_step(None, 1, 4, *h, 1, None) == _lib.TS_EINVAL
    assert L.ts_adamw_multi_step(a, 0, 4, *h, 1, None) == _lib.TS_EINVAL and L.ts_adamw_multi_step(a, 1, 0, *h, 1, None) == _lib.TS_EINVAL


def test_fused_adamw_keeps_the_bf16_shadows_current():
    from thunder_speech_amd.optim import FusedAdamW
    from thunder_speech_amd.train_ops import bf16_shadow
    g = torch.Generator().manual_seed(4)
    shapes = [(29, 64, 1), (29,), (5, 7), (1003,), (64, 33), (16, 1, 33), (64,), (64,), (48, 16, 1), (3, 1025)]
    ps = [torch.nn.Parameter(torch.randn(s, generator=g).cuda()) for s in shapes]
    shadows = {i: bf16_shadow(p, create=True) for i, p in enumerate(ps) if p.dim() >= 2}
    assert len(ps) >= 8 and len(shadows) >= 5 and all(s[1] == -1 for s in shadows.values())
    opt = FusedAdamW(ps, lr=1e-2)
    for step in range(3):
        before = [p.detach().clone() for p in ps]
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g).cuda()
        opt.step()
        torch.cuda.synchronize()
        for i, p in enumerate(ps):
            assert not torch.equal(p.detach(), before[i])
            ent = bf16_shadow(p)
            assert (ent is not None) == (i in shadows)
            if ent is not None:
                assert ent is shadows[i] and ent[1] == p._version, f"step {step} parameter {i}: the shadow is not marked current"
                assert torch.equal(ent[0].view(torch.int16).flatten(), p.detach().to(BF).view(torch.int16).flatten()), f"step {step} parameter {i}: stale shadow"


def torch_adamw_double(p, grad, m, v, lr, betas, eps, wd, step):
    """one step of torch.optim.AdamW in float64 with double hyper-parameters, entered at `step` with the given moments"""
    q = torch.nn.Parameter(p.double().clone())
    q.grad = grad.double().clone()
    opt = torch.optim.AdamW([q], lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=False)
    opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.double().clone(), "exp_avg_sq": v.double().clone()}
    opt.step()
    return q.detach()


def beta2_first_order(b2, step):
    """relative change of c2 = 1 - b2^s when b2 is rounded to f32: s b2^(s-1) |f32(b2) - b2| / c2"""
    return step * b2 ** (step - 1) * abs(f32(b2) - b2) / (1.0 - b2 ** step)


@pytest.mark.parametrize("step", [1, 100, 1000])
def test_adamw_step_deviates_from_double_torch_by_the_rounding_of_its_hyper_parameters_only(step):
    from thunder_speech_amd import _lib
    L = _lib.lib()
    n = 4099
    lr, betas, eps, wd = 1e-3, (0.9, 0.999), 1e-8, 1e-2
    ops = adamw_operands(n, 7 + step)
    want = torch_adamw_double(*ops, lr, betas, eps, wd, step)
    r32 = adamw_restate(*[o.double() for o in ops], f32(lr), f32(betas[0]), f32(betas[1]), f32(eps), f32(wd), step)
    r64 = adamw_restate(*[o.double() for o in ops], lr, betas[0], betas[1], eps, wd, step, bound=False)
    assert float((r64["p"] - want).abs().max()) <= 1e-13 * float(want.abs().max())                # the restatement is torch's formula
    derived = (r32["p"] - r64["p"]).abs()
    d = [o.cuda() for o in ops]
    assert L.ts_adamw_step(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n, lr, betas[0], betas[1], eps, wd, step, _stream()) == 0
    torch.cuda.synchronize()
    measured = (d[0].cpu().double() - want).abs()
    upd = r64["upd"].abs()
    moving = upd > 0
    print(f"RATIO|adamw-vs-torch|step={step}|measured / update: max {float((measured[moving] / upd[moving]).max()):.3e} median "
          f"{float((measured[moving] / upd[moving]).median()):.3e}|derived / update: max {float((derived[moving] / upd[moving]).max()):.3e} median "
          f"{float((derived[moving] / upd[moving]).median()):.3e}|first order in beta2: dc2 / c2 = {beta2_first_order(betas[1], step):.3e}")
    _report("adamw-vs-torch", f"step={step}", measured, derived + r32["dp"])


# ---------------------------------------------------------------------------------------------------------------------
# 11. ts_audio_prep
# ---------------------------------------------------------------------------------------------------------------------
def resample_geometry(rate, target=16000):
    gcd = math.gcd(rate, target)
    return rate // gcd, target // gcd


def audio_prep_restate(audio, kern, orig, new, width):
    """audio f32 [C][t], kern f32 [new][kw] or None -> (out, bound) float64 [t_out]"""
    ch, t = audio.shape
    a = audio.double()
    mono = a.mean(0)
    d_mono = gam(ch + 2) * a.abs().mean(0) if ch > 1 else torch.zeros_like(mono)
    mean = mono.mean()
    d_mean = d_mono.mean() + t * 2.0 ** -53 * mono.abs().mean() + U * mean.abs()
    x = mono - mean
    d_x = d_mono + d_mean + gam(1) * (x.abs() + d_mono + d_mean)
    if not bool(audio.any()):
        d_x = torch.zeros_like(x)                                       # exact zeros: every intermediate is exactly 0
    if kern is None:
        return x, d_x
    k = kern.double()
    kw = k.shape[1]
    assert kw == 2 * width + orig and k.shape[0] == new
    t_out = math.ceil(new * t / orig)
    conv = lambda sig, ker: F.conv1d(F.pad(sig, (width, width + orig))[None, None], ker[:, None, :], stride=orig)[0].transpose(0, 1).reshape(-1)[:t_out]
    out = conv(x, k)
    bound = conv(d_x, k.abs()) + gam(kw) * conv(x.abs() + d_x, k.abs())
    return out, bound


def audio_clip(channels, t, seed, zeros=False):
    if zeros:
        return torch.zeros(channels, t)
    a = 0.3 * torch.randn(channels, t, generator=torch.Generator().manual_seed(seed)) + 0.1
    if t >= 64:
        a[:, t // 3: t // 3 + 20] = 0.0
    return a


AUDIO_CASES = [(1, 16000, 1), (1, 16000, 4095), (1, 16000, 4096), (2, 16000, 4097), (1, 8000, 1), (1, 8000, 5), (3, 44100, 3), (1, 44100, 441), (2, 22050, 8193),
               (1, 48000, 12289)]


@pytest.mark.parametrize("channels,rate,t", AUDIO_CASES)
def test_audio_prep_matches_the_float64_restatement(channels, rate, t):
    from thunder_speech_amd import _lib
    from thunder_speech_amd.data.dataset import _sinc_kernel
    L = _lib.lib()
    kern, width, orig, new = (None, 0, 1, 1) if rate == 16000 else _sinc_kernel(rate, 16000)
    assert (orig, new) == resample_geometry(rate) or kern is None
    kd = kern.cuda() if kern is not None else None
    t_out = t if kern is None else math.ceil(new * t / orig)
    ws_bytes = L.ts_audio_prep_workspace_bytes(t)
    assert ws_bytes >= 4 * t + 8 * ((t + 4095) // 4096)
    for zeros in (False, True):
        what = f"audio prep C={channels} rate={rate} t={t} zeros={zeros}"
        audio = audio_clip(channels, t, rate + t, zeros)
        ad = audio.cuda()
        runs = []
        for _ in range(2):
            wsbuf = torch.full((ws_bytes + 2048,), 255, dtype=torch.uint8, device="cuda")
            ws = wsbuf[1024: 1024 + ws_bytes]
            buf, out = _flat(t_out, torch.float32, NAN, GUARD)
            st = L.ts_audio_prep(ad.data_ptr(), channels, t, kd.data_ptr() if kd is not None else None, orig, new, kern.shape[1] if kern is not None else 0, width,
                                 out.data_ptr(), t_out, ws.data_ptr(), _stream())
            assert st == 0, what
            torch.cuda.synchronize()
            _flat_ok(buf, t_out, GUARD, what)
            assert bool((wsbuf[:1024] == 255).all()) and bool((wsbuf[1024 + ws_bytes:] == 255).all()), f"{what}: bytes next to the workspace were written"
            runs.append(out.cpu())
        assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), f"{what}: two calls differ"
        ref, bound = audio_prep_restate(audio, kern, orig, new, width)
        assert ref.numel() == t_out
        _report("audio-prep", what, (runs[0].double() - ref).abs(), bound)
        if zeros:
            assert bool((runs[0] == 0).all())
        assert torch.equal(ad.cpu(), audio)
    E = _lib.TS_EINVAL
    a = out.data_ptr()
    assert L.ts_audio_prep(None, 1, 4, None, 1, 1, 0, 0, a, 4, a, None) == E and L.ts_audio_prep(a, 1, 4, None, 1, 1, 0, 0, a, 5, a, None) == E
    assert L.ts_audio_prep(a, 1, 4, None, 1, 1, 0, 0, a, 4, None, None) == E and L.ts_audio_prep(a, 0, 4, None, 1, 1, 0, 0, a, 4, a, None) == E
    assert L.ts_audio_prep(a, 1, 4, a, 0, 1, 3, 1, a, 4, a, None) == E and L.ts_audio_prep_workspace_bytes(0) == E


# ---------------------------------------------------------------------------------------------------------------------
# 12. ts_decoder_bwd
# ---------------------------------------------------------------------------------------------------------------------
def decoder_bwd_restate(gl, x):
    """gl f32 [b][v][t], x bf16 [b][c][t] -> (dW [v][c], its bound, db [v], its bound) float64"""
    b, _, t = gl.shape
    g64, x64 = gl.double(), x.double()
    k = gam(t * b + b + 1)
    return (torch.einsum("bvt,bct->vc", g64, x64), k * torch.einsum("bvt,bct->vc", g64.abs(), x64.abs()), g64.sum(dim=(0, 2)), k * g64.abs().sum(dim=(0, 2)))


@pytest.mark.parametrize("b,v,c,t", [(1, 1, 1, 1), (2, 32, 64, 128), (2, 33, 65, 129), (3, 29, 63, 127), (1, 64, 128, 256), (5, 29, 200, 301)])
def test_decoder_bwd_matches_the_float64_einsum(b, v, c, t):
    from thunder_speech_amd import _lib
    L = _lib.lib()
    g = torch.Generator().manual_seed(b * 1000 + t)
    x = torch.randn(b, c, t, generator=g).to(BF)
    gl = torch.randn(b, v, t, generator=g)
    pitch_x, pitch_g = (t + 8) // 8 * 8 + 8, t + 3
    xd = torch.full((b, c, pitch_x), PAD, dtype=BF, device="cuda")
    xd[:, :, :t] = x.cuda()
    gd = torch.full((b, v, pitch_g), PAD, device="cuda")
    gd[:, :, :t] = gl.cuda()
    ref_w, e_w, ref_b, e_b = decoder_bwd_restate(gl, x)
    what = f"decoder bwd b={b} v={v} c={c} t={t}"
    runs = []
    for _ in range(2):
        wbuf, dw = _flat(v * c, torch.float32, 7.0, GUARD)
        bbuf, db = _flat(v, torch.float32, 7.0, GUARD)
        st = L.ts_decoder_bwd(gd.data_ptr(), xd.data_ptr(), b, v, c, t, pitch_g, pitch_x, dw.data_ptr(), db.data_ptr(), _stream())
        assert st == 0, what
        torch.cuda.synchronize()
        _flat_ok(wbuf, v * c, GUARD, what + " dW")
        _flat_ok(bbuf, v, GUARD, what + " db")
        runs.append((dw.cpu().double().view(v, c), db.cpu().double()))
        _report("decoder-bwd-dw", what, (runs[-1][0] - ref_w).abs(), e_w)
        _report("decoder-bwd-db", what, (runs[-1][1] - ref_b).abs(), e_b)
    _report("decoder-bwd-rerun", what, (runs[0][0] - runs[1][0]).abs(), 2 * e_w)
    _report("decoder-bwd-rerun", what, (runs[0][1] - runs[1][1]).abs(), 2 * e_b)
    E = _lib.TS_EINVAL
    a = dw.data_ptr()
    for args in [(None, a, 1, 1, 1, 4, 4, 4, a, a), (a, None, 1, 1, 1, 4, 4, 4, a, a), (a, a, 1, 1, 1, 4, 4, 4, None, a), (a, a, 1, 1, 1, 4, 4, 4, a, None),
                 (a, a, 0, 1, 1, 4, 4, 4, a, a), (a, a, 1, 1, 1, 4, 3, 4, a, a), (a, a, 1, 1, 1, 4, 4, 3, a, a)]:
        assert L.ts_decoder_bwd(*args, None) == E, args
