"""The mel front end (csrc/frontend.hip: stft_mel_kernel<dither>, normalize_kernel) behind ts_mel_frontend_fwd and the five stage kernels ts_fe_*
(csrc/frontend_stages.hip), launched through the C ABI and compared per element with plain float64 restatements on the CPU (torch.stft, conv1d, matmul,
log in float64; nothing of thunder_speech_amd or oracle takes part in the arithmetic -- the oracle's Slaney bank is read as data).  Every fused case
asserts what ts_frontend_launch_config says it launches: the persistent grid, the number of frame groups it walks and the instantiation.

Restatement, from the operands the device holds (f32 waveform, f32 window[512], preemph rounded to f32, f32 CSR weights and offsets, int32 lengths;
with dither the f32 noise the device's own ts_fe_dither leaves on zeros with dither = 1 -- the same pure function of (seed, clip, sample)):
x (+ dither x noise); pre-emphasis pe[k] = x[k] - p x[k - 1], pe[0] = x[0]; reflect padding by 256 at n_samples, not at the clip's length;
torch.stft in float64; P = |X|^2; mel = CSR product; logmel = log(mel + 2^-24); flen = len // hop + 1; over the n = min(flen, n_frames) valid frames
mu = mean, var = (sum (logmel - mu)^2 + (n_frames - n) mu^2) / n (quirk A1), z = (logmel - mu) / (sqrt(var) + 1e-5); frames >= n, mask rectangles and
the columns [n_frames, pitch) are 0.  test_restatement_matches_the_reference_fixtures (no gpu mark) pins it against tests/golden/frontend_{qn,cn}.npz.

Bound, per element (u = u32 = 2^-24, u16 = 2^-8), from the roundings between operands and store.  Nothing is fitted to measured ratios (profiles/
frontend_ctc_se_kernel_checks.md has those):
  input     sig = xc - p xp: a product and a difference (one rounding if contracted to an fma):   d_sig = u (|p xp| + |sig|)
            with dither each of xc, xp is x + d noise first: a product, an add, and one ulp for the noise being evaluated in another kernel:
                                                                                                   d_x = u (2 |d noise| + |x|)
            y = sig win, one rounding:                                                             d_y = |win| d_sig + u |y|
            A perturbation dy of the frame moves every bin by at most sum_j |dy_j|:                e_in = sum_j d_y[j]
  spectrum  the 512-point real FFT is a 256-point complex FFT of z[n] = y[2n] + i y[2n + 1] (four-step, 16 x 16) and the real-FFT split.  Every
            level is a scaled unitary map, so a relative error c u committed in the 2-norm at one level arrives at the output as c u ||Z||_2,
            ||Z||_2 = 16 ||y||_2, and |dZ_k| + |dZ_{256-k}| <= sqrt(2) ||dZ||_2: a bin of X sees c u sqrt(512) ||y||_2.  Counting c from the code:
              fft16: two levels of complex adds per radix-4 stage (u each), two stages: 4; its inner twiddles W16 are f32 constants (u) and a
                     complex product costs (1 + sqrt 2) u < 3 u in norm (two products and an add, or product and fma, per component): 4    -> 8
              two fft16 calls                                                                                                          -> 16
              inter-stage twiddle: the table comes from sincospif (2 ulp = 4 u), one complex product (3 u)                             ->  7
              split, relative to |Z_k| + |Z_{256-k}| <= sqrt(512) ||y||_2: A and D one add each (u); w = tw x w_odd: 4 u + u + 3 u = 8 u;
                     wd = D w: u + 8 u + 3 u = 12 u; X = (A + rot(wd)) / 2: (u + 12 u + 2 u) / 2 = 7.5 u                               ->  8
            K = 31:                                                                                eta = e_in + K u sqrt(512) ||y||_2
            (a float32 FFT on a CPU reaches about 0.58 u sqrt(512) ||y||_2: the worst case sits some 50 times above a typical error)
  power     P = xr xr + xi xi, three roundings at most:                                           dP = 2 |X| eta + eta^2 + 3 u (P + 2 |X| eta + eta^2)
  mel sum   cnt fused multiply-adds and the add of the floor:                                      dmel = sum w dP + (cnt + 1) u sum w (P + dP)
  log       of the perturbed argument, v = mel + 2^-24:                                            -log1p(-dmel / v)
            logf under -ffast-math is v_log_f32 (1 ulp = 2 u of log2 v) times the f32 constant ln 2 (u) rounded (u), and one ulp at 1:
                                                                                                   E_lm = -log1p(-dmel / v) + 4 u |logmel| + 2 u
  normaliser  (e1, a1: means of E_lm and |logmel| over the n valid frames; var = sum (logmel - mu)^2 / n + (n_frames - n) / n mu^2)
            the perturbation E_lm of the log-mel moves the mean by at most e1 and, through the exact expression of the variance, var by
                                       p_var = mean(2 |logmel - mu| (E_lm + e1) + (E_lm + e1)^2) + (n_frames - n) / n (2 |mu| e1 + e1^2)
            the kernel sums 16 frames at a time in f32 (each term through at most k = min(16, n) roundings), the rest in f64, and forms
            s2 / n + c mu^2 with c = (n_frames - 2 n) / n -- the s2 - n mu^2 cancellation: the two roundings enter as absolute errors of terms of the
            size of logmel^2           r1 = k u (a1 + e1),   r2 = k u mean((|logmel| + E_lm)^2)
                                       d_mu = e1 + r1,   d_var = p_var + r2 + |c| (2 (|mu| + e1) r1 + r1^2)
                                       d_sigma = min(d_var / sigma, sqrt(d_var))                                    (the 1 / sigma stays)
            rs = 1 / (sigma + 1e-5), q = rs d_sigma:                                               d_rs = rs q / (1 - q) + 2 u rs
            mean rounded to f32, the difference and the product rounded:                           t = E_lm + d_mu + u (|mu| + d_mu); t += u (|logmel - mu| + t)
                                                                                                   E_z = t (rs + d_rs) + |logmel - mu| d_rs; E_z += u (|z| + E_z)
  store     bf16, round to nearest even:                                                           E = E_z + u16 (|z| + E_z)
  Frames at or beyond the length, mask rectangles and [n_frames, pitch) have bound 0: they must be exactly 0.
Condition on the inputs, asserted for every case: dmel <= (mel + 2^-24) / 4 everywhere, and sigma > 0 with q <= 1 / 2 for every (clip, mel) row whose
valid log-mel frames are not all equal with n = n_frames -- a row whose true sigma is 0 (a fully silent full-length clip, a mel row without weights) is
rounding noise amplified by 1e5 in any implementation: its log-mel is checked, its features only where they must be 0.

Conventions as in tests/test_gpu_tcs_kernels.py: return codes asserted; features inside a NaN-filled buffer with guard rows of 7.0, the workspace
between guard bytes, feat_len / feat_len64 between sentinels, all of which must come back bit for bit; `RATIO|kind|error / bound` printed before every
assert; no element left out."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

NAN = float("nan")
BF = torch.bfloat16
GUARD = 7.0
GUARD_ROWS = 8
GUARD_BYTES = 1024
U16 = 2.0 ** -8
U32 = 2.0 ** -24
FLOOR = 2.0 ** -24
NFFT = 512
K_FFT = 31
LOG_FLOOR = float(torch.log(torch.tensor(FLOOR, dtype=torch.float64)))
HERE = os.path.dirname(os.path.abspath(__file__))


def _report(kind, what, err, bound):
    ratio = float((err / bound.clamp_min(1e-300)).max()) if bool((bound > 0).any()) else 0.0
    worst = int((err - bound).argmax())
    print(f"RATIO|{kind}|{ratio:.3e}|{what}")
    assert not bool(torch.isnan(err).any()), f"{what}: unwritten (NaN) elements"
    assert bool((err <= bound).all()), (f"{what}: error {float(err.flatten()[worst]):.3e} > bound {float(bound.flatten()[worst]):.3e} at flat index {worst} "
                                        f"(largest error / bound {ratio:.3e})")
    return ratio


# ---------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------
def _window(win_length):
    w = torch.zeros(NFFT)
    left = (NFFT - win_length) // 2
    w[left: left + win_length] = torch.hann_window(win_length, periodic=False)
    return w


def _csr(fb):
    """dense f32 [n_mels][257] -> (weights f32, offsets int32 [n_mels + 1][2]) as quartznet/transform.py packs them: first to last non-zero bin"""
    weights, offsets = [], []
    for m in range(fb.shape[0]):
        nz = torch.nonzero(fb[m]).flatten()
        first, last = (int(nz[0]), int(nz[-1]) + 1) if len(nz) else (0, 0)
        offsets.append((first, len(weights)))
        weights.extend(fb[m, first:last].tolist())
    offsets.append((0, len(weights)))
    return torch.tensor(weights, dtype=torch.float32).reshape(-1), torch.tensor(offsets, dtype=torch.int32)


def _slaney(n_mels):
    from oracle.frontend import slaney_mel_filterbank                      # data: the bank both model families use
    return torch.from_numpy(slaney_mel_filterbank(NFFT // 2 + 1, n_mels, 16000))


def _synthetic_bank(n_mels):
    """Sparse positive bank: row 0 without weights, row 1 one weight, rows 2 and 3 wide (200 and 257 bins), the last row ending at bin 256, the others
    narrow triangles walking up the spectrum"""
    g = torch.Generator().manual_seed(n_mels)
    fb = torch.zeros(n_mels, NFFT // 2 + 1)
    for m in range(n_mels):
        first = (m * 253) // n_mels
        width = 1 + int(torch.randint(1, 12, (1,), generator=g))
        fb[m, first: min(first + width, 257)] = 0.002 + 0.02 * torch.rand(min(first + width, 257) - first, generator=g)
    fb[0] = 0
    if n_mels > 4:
        fb[1] = 0
        fb[1, 7] = 0.03
        fb[2] = 0
        fb[2, 20:220] = 0.001 + 0.002 * torch.rand(200, generator=g)
        fb[3] = 0.0005 + 0.001 * torch.rand(257, generator=g)
    fb[n_mels - 1] = 0
    fb[n_mels - 1, 250:257] = 0.01 + 0.01 * torch.rand(7, generator=g)
    return fb


def _case(name, n, lens, **kw):
    d = dict(name=name, n=n, lens=lens, hop=160, win=320, n_mels=64, bank="slaney", dither=0.0, seed=0, masks=None, offset=0, amp=0.3, silent=(),
             batch_from_grid=None, pitch=None, ramp=False)
    d.update(kw)
    return d


def _r8(x):
    return (x + 7) // 8 * 8


LONG_LENS = lambda n: [0, 1, 159, 160, n - 1, n, n + 5, n - 160]       # n makes the last frame valid (flen = n_frames); n - 160 makes it the first invalid one
CASES = [
    # ---- the persistent loop in its steady state: batch from the query, n_groups >= 3 x grid (short) and >= 2 x grid + 5 (long)
    _case("steady-short", 6400, None, batch_from_grid=("plus", 3, 3.0), silent=(1,)),
    _case("steady-long", 48000, LONG_LENS(48000), batch_from_grid=("groups", 5, 2.0)),
    _case("steady-dither", 6400, None, batch_from_grid=("plus", 3, 3.0), dither=1e-5, seed=0x1234567890ABCDEF),
    # ---- direct staging only
    _case("direct-n6401", 6401, [6401, 3000, 161]),
    _case("direct-n6402", 6402, [6402, 3000, 0]),
    _case("direct-n6403", 6403, [6403, 6402, 320]),
    _case("direct-base-plus-4-bytes", 6400, [6400, 3000, 161], offset=1),
    _case("direct-hop171", 6400, [6400, 3000, 171], hop=171),
    _case("direct-hop200", 6400, [6400, 3000, 199], hop=200),
    # ---- vector staging at its limit
    _case("vector-hop170", 6400, [6400, 3000, 170], hop=170),
    _case("vector-hop100", 6400, [6400, 3000, 99], hop=100),
    # ---- mel geometry
    _case("citrinet-80-win400", 6400, [6400, 3000, 161], n_mels=80, win=400),
    _case("mels-1", 6400, [6400, 3000, 161], n_mels=1),
    _case("mels-247", 6400, [6400, 3000, 161], n_mels=247, bank="synthetic"),
    _case("mels-248", 6400, [6400, 3000, 161], n_mels=248, bank="synthetic"),
    _case("mels-256", 6400, [6400, 3000, 161], n_mels=256, bank="synthetic"),
    # ---- shortest input: both reflections inside frame 1
    _case("shortest-257", 257, [257, 160, 0], ramp=True),                 # its two frames share most samples: a ramp keeps their log-mel apart (sigma > 0)
    # ---- masks: at frame 0 and mel 0, across an 8-frame store group, across the 64-frame tile border, beyond the length, empty ones
    _case("masks", 16000, [16000, 9000, 161], masks=[(0, 3, 0, 5), (10, 20, 6, 10), (30, 40, 60, 70), (0, 64, 95, 200), (5, 5, 10, 20), (5, 9, 20, 20),
                                                   (60, 64, 100, 101)]),
    # ---- the library's own pitch
    _case("time-pitch", 6400, [6400, 3000, 161], pitch="time_pitch", silent=()),
]


def _desc_fields(case, batch):
    n, hop = case["n"], case["hop"]
    n_frames = n // hop + 1
    return dict(batch=batch, n_samples=n, n_fft=NFFT, hop=hop, win_length=case["win"], n_mels=case["n_mels"], preemph=0.97, n_frames=n_frames,
                pitch_out=_r8(n_frames + 72), dither=case["dither"], dither_seed=case["seed"])


def _tables(case):
    fb = _slaney(case["n_mels"]) if case["bank"] == "slaney" else _synthetic_bank(case["n_mels"])
    mw, moff = _csr(fb)
    return _window(case["win"]), fb, mw, moff


def _wave(case, batch):
    """Gaussian noise of amplitude <= amp with a stretch of exact zeros in every clip (the spectrum of a frame inside it is exactly 0); the clips
    named by case["silent"] are all zeros.  Lengths: the case's, or cycled."""
    n = case["n"]
    g = torch.Generator().manual_seed(len(case["name"]) + n)
    x = (case["amp"] / 3.0) * torch.randn(batch, n, generator=g)
    x = x.clamp(-case["amp"], case["amp"])
    if case["ramp"]:
        x = x * torch.linspace(0.02, 1.0, n)[None, :]
    if n >= 3000:
        starts = torch.randint(0, n - 1400, (batch,), generator=g)
        idx = torch.arange(n)[None, :]
        x[(idx >= starts[:, None]) & (idx < starts[:, None] + 1400)] = 0.0
    for i in case["silent"]:
        x[i] = 0.0
    if case["lens"] is None:
        cyc = [n, 0, n - 1, 3000, 161, 160, 159, n + 5]
        lens = [cyc[i % len(cyc)] for i in range(batch)]
        for i in case["silent"]:
            lens[i] = n
    else:
        lens = [case["lens"][i % len(case["lens"])] for i in range(batch)]
    return x, torch.tensor(lens, dtype=torch.int32)


# ---------------------------------------------------------------------------------------------------------------------
# float64 restatement and bound
# ---------------------------------------------------------------------------------------------------------------------
def _restate(x, lens, win, mw, moff, hop, preemph, masks=None, noise=None, dither=0.0):
    """x f32 [B][n], lens int32 [B], win f32 [512], CSR (mw, moff) -> dict of float64 tensors: logmel [B][M][F] with its bound, features z [B][M][F] with
    its bound, flen [B], degenerate [B][M] (true sigma 0).  Asserts the conditions on the inputs."""
    b, n = x.shape
    p = float(np.float32(preemph))
    xd = x.double()
    e_x = torch.zeros_like(xd)
    if dither:
        d = float(np.float32(dither))
        dn = d * noise.double()
        xd = xd + dn
        e_x = U32 * (2 * dn.abs() + xd.abs())
    pe, e_pe = xd.clone(), e_x.clone()
    pe[:, 1:] = xd[:, 1:] - p * xd[:, :-1]
    e_pe[:, 1:] = e_x[:, 1:] + p * e_x[:, :-1] + U32 * ((p * xd[:, :-1]).abs() + pe[:, 1:].abs())
    pad = F.pad(pe[:, None, :], (NFFT // 2, NFFT // 2), mode="reflect")
    e_pad = F.pad(e_pe[:, None, :], (NFFT // 2, NFFT // 2), mode="reflect")
    w = win.double()
    spec = torch.stft(pad[:, 0], NFFT, hop, NFFT, window=w, center=False, return_complex=True)          # [B][257][F]
    nf = spec.shape[-1]
    assert nf == n // hop + 1
    wk = w.abs()[None, None, :]
    sum_abs_y = F.conv1d(pad.abs(), wk, stride=hop)[:, 0]                                                # [B][F]
    norm_y = F.conv1d(pad * pad, wk * wk, stride=hop)[:, 0].clamp_min(0).sqrt()
    e_in = F.conv1d(e_pad, wk, stride=hop)[:, 0] + U32 * sum_abs_y
    eta = (e_in + K_FFT * U32 * math.sqrt(NFFT) * norm_y)[:, None, :]                                    # [B][1][F]
    ax = spec.abs()
    pw = ax * ax
    dp = 2 * ax * eta + eta * eta
    dp = dp + 3 * U32 * (pw + dp)
    n_mels = moff.shape[0] - 1
    bank = torch.zeros(n_mels, NFFT // 2 + 1, dtype=torch.float64)
    cnt = torch.zeros(n_mels, dtype=torch.float64)
    for m in range(n_mels):
        first, off = int(moff[m, 0]), int(moff[m, 1])
        c = int(moff[m + 1, 1]) - off
        assert 0 <= c and first + c <= NFFT // 2 + 1 and (c == 0 or bool((mw[off: off + c] >= 0).all()))
        bank[m, first: first + c] = mw[off: off + c].double()
        cnt[m] = c
    mel = torch.einsum("mk,bkf->bmf", bank, pw)
    dmel = torch.einsum("mk,bkf->bmf", bank, dp)
    dmel = dmel + (cnt[None, :, None] + 1) * U32 * (mel + dmel)
    dmel = torch.where(cnt[None, :, None] > 0, dmel, torch.zeros_like(dmel))                             # no weights: the sum is the exact 0
    v = mel + FLOOR
    assert bool((dmel <= v / 4).all()), f"input condition: dmel / (mel + 2^-24) reaches {float((dmel / v).max()):.3f}"
    lm = torch.log(v)
    e_lm = -torch.log1p(-dmel / v) + 4 * U32 * lm.abs() + 2 * U32
    flen = torch.div(lens.long(), hop, rounding_mode="floor") + 1
    nv = flen.clamp(max=nf)
    valid = (torch.arange(nf)[None, :] < nv[:, None])[:, None, :]                                        # [B][1][F]
    nn = nv.double()[:, None, None]
    vm = valid.double()
    mean = lambda t: (t * vm).sum(-1, keepdim=True) / nn
    mu, a1, e1 = mean(lm), mean(lm.abs()), mean(e_lm)
    k16 = nn.clamp(max=16)                                                                               # terms of one group's partial sum
    r1 = k16 * U32 * (a1 + e1)
    d_mu = e1 + r1
    r2 = k16 * U32 * mean((lm.abs() + e_lm) ** 2)
    c = (nf - 2 * nn) / nn
    var = (((lm - mu) ** 2 * vm).sum(-1, keepdim=True) + (nf - nn) * mu * mu) / nn
    dev = e_lm + e1
    d_var = mean(2 * (lm - mu).abs() * dev + dev * dev) + (nf - nn) / nn * (2 * mu.abs() * e1 + e1 * e1) + r2 + c.abs() * (2 * (mu.abs() + e1) * r1 + r1 * r1)
    sigma = var.clamp_min(0).sqrt()
    d_sigma = torch.minimum(d_var / sigma.clamp_min(1e-300), d_var.sqrt())
    rs = 1.0 / (sigma + 1e-5)
    q = rs * d_sigma
    big = torch.where(valid, lm, torch.full_like(lm, -1e30)).max(-1, keepdim=True).values
    small = torch.where(valid, lm, torch.full_like(lm, 1e30)).min(-1, keepdim=True).values
    degenerate = (big == small) & (nn == nf)                                                              # the true sigma is 0
    assert bool((degenerate | ((sigma > 0) & (q <= 0.5))).all()), f"input condition: rs x d_sigma reaches {float(q[~degenerate].max()):.3f}"
    qc = q.clamp(max=0.5)
    d_rs = rs * qc / (1 - qc) + 2 * U32 * rs
    diff = lm - mu
    z = diff * rs
    t = e_lm + d_mu + U32 * (mu.abs() + d_mu)
    t = t + U32 * (diff.abs() + t)
    e_z = t * (rs + d_rs) + diff.abs() * d_rs
    e_z = e_z + U32 * (z.abs() + e_z)
    e = e_z + U16 * (z.abs() + e_z)
    keep = valid.expand_as(z).clone()
    for (f0, f1, t0, t1) in masks or ():
        keep[:, max(f0, 0): max(f1, 0), max(t0, 0): max(t1, 0)] = False
    z, e = z * keep, e * keep
    return dict(logmel=lm, e_logmel=e_lm, z=z, e_z=e, flen=flen, degenerate=degenerate[:, :, 0], keep=keep, sigma=sigma[:, :, 0])


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the restatement against the reference's fixtures; the conditions on the inputs of every case that needs no device noise
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,win,n_mels", [("qn", 320, 64), ("cn", 400, 80)])
def test_restatement_matches_the_reference_fixtures(golden, tag, win, n_mels):
    """tests/golden/frontend_{qn,cn}.npz were written by the reference's own modules; the tolerances are those of
    tests/test_gpu_frontend_decode_ctc.py::test_frontend_matches_reference_fixture (the fixtures are f32 results)."""
    g = golden(f"frontend_{tag}.npz")
    x = torch.from_numpy(g["x"])
    lens = torch.from_numpy(g["lengths"]).to(torch.int32)
    mw, moff = _csr(_slaney(n_mels))
    r = _restate(x, lens, _window(win), mw, moff, 160, 0.97)
    assert np.array_equal(r["flen"].numpy(), g["feat_lengths"])
    np.testing.assert_allclose(r["logmel"].numpy(), g["logmel"], atol=2e-3)
    np.testing.assert_allclose(r["z"].numpy(), g["features"], atol=2e-2)
    assert not bool(r["degenerate"].any())


def _host_grid(L, _lib, case, batch, tables, keep):
    d = _lib.FrontendDesc(**_desc_fields(case, batch))
    win, fb, mw, moff = tables
    keep += [win, mw, moff]
    d.window, d.mel_weights, d.mel_offsets, d.mel_nnz = win.data_ptr(), mw.data_ptr(), moff.data_ptr(), mw.numel()
    out = [C.c_int32(-7) for _ in range(4)]
    st = L.ts_frontend_launch_config(C.byref(d), *[C.byref(o) for o in out])
    return st, tuple(o.value for o in out)


def _batch_for(case, query):
    """steady-state cases size their batch from the query: ("plus", k, f): batch = grid + k; ("groups", k, f): n_groups >= f x grid + k"""
    if case["batch_from_grid"] is None:
        return len(case["lens"])
    kind, k, _ = case["batch_from_grid"]
    st, (grid, n_groups, _, _) = query(4096)
    assert st == 0 and grid < n_groups
    nwg = (case["n"] // case["hop"] + 1 + 15) // 16
    return grid + k if kind == "plus" else (2 * grid + k + nwg - 1) // nwg


@pytest.mark.parametrize("case", [c for c in CASES if not c["dither"]], ids=[c["name"] for c in CASES if not c["dither"]])
def test_inputs_satisfy_the_conditions_of_the_bound(case):
    """dmel <= (mel + 2^-24) / 4 and sigma > 0 (asserted inside _restate) for the inputs of every case, without a GPU; the launch query answers on the
    host too (256 CUs and the LDS limit assumed without a device), and the steady-state batches it gives satisfy the cases' group counts."""
    from thunder_speech_amd import _lib
    L = _lib.lib()
    tables = _tables(case)
    keep = []
    query = lambda batch: _host_grid(L, _lib, case, batch, tables, keep)
    batch = _batch_for(case, query)
    st, (grid, n_groups, lds, di) = query(batch)
    assert st == 0 and di == 0 and n_groups == batch * ((case["n"] // case["hop"] + 1 + 15) // 16) and 0 < grid <= n_groups and lds > 0
    if case["batch_from_grid"]:
        assert n_groups >= case["batch_from_grid"][2] * grid + (case["batch_from_grid"][1] if case["batch_from_grid"][0] == "groups" else 0)
        batch = min(batch, 64)                                             # the inputs are drawn per clip: a slice of the batch says as much here
    x, lens = _wave(case, batch)
    win, fb, mw, moff = tables
    r = _restate(x, lens, win, mw, moff, case["hop"], 0.97, masks=case["masks"])
    assert float(r["logmel"].min()) == LOG_FLOOR or case["n"] < 3000     # frames inside the stretch of zeros: the spectrum is exactly 0
    if case["bank"] == "synthetic":
        off = moff[:, 1].tolist()
        counts = [off[i + 1] - off[i] for i in range(case["n_mels"])]
        assert counts[0] == 0 and counts[1] == 1 and counts[2] == 200 and counts[3] == 257 and int(moff[case["n_mels"] - 1, 0]) + counts[-1] == 257
        assert bool(r["degenerate"][0, 0]) and not bool(r["degenerate"][1:].any()) and not bool(r["degenerate"][0, 1:].any())


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the fused front end
# ---------------------------------------------------------------------------------------------------------------------
def _stream():
    return torch.cuda.current_stream().cuda_stream


def _run_fused(L, _lib, case, batch, tables, x, lens):
    """-> (status, logmel [B][F][M] f32, features [B][M][pitch] f32, feat_len, feat_len64, noise or None), all on the CPU, guards checked"""
    win, fb, mw, moff = tables
    fields = _desc_fields(case, batch)
    if case["pitch"] == "time_pitch":
        fields["pitch_out"] = _lib.time_pitch(fields["n_frames"])
    n, nf, nm, pitch = case["n"], fields["n_frames"], case["n_mels"], fields["pitch_out"]
    assert pitch >= nf + 72
    d = _lib.FrontendDesc(**fields)
    wd, mwd, moffd = win.cuda(), mw.cuda(), moff.cuda()
    d.window, d.mel_weights, d.mel_offsets, d.mel_nnz = wd.data_ptr(), mwd.data_ptr(), moffd.data_ptr(), mw.numel()
    md = None
    if case["masks"]:
        md = torch.tensor(case["masks"], dtype=torch.int32).cuda()
        d.masks, d.n_masks = md.data_ptr(), len(case["masks"])
    flat = torch.full((batch * n + 4 + case["offset"],), NAN, device="cuda")
    xd = flat[case["offset"]: case["offset"] + batch * n].view(batch, n)
    xd.copy_(x.cuda())
    assert xd.data_ptr() % 16 == 4 * case["offset"]
    ld = lens.cuda()
    noise = None
    if case["dither"]:
        zeros = torch.zeros(batch, n, device="cuda")
        nd = torch.full((batch, n), NAN, device="cuda")
        assert L.ts_fe_dither(zeros.data_ptr(), nd.data_ptr(), batch, n, 1.0, case["seed"], _stream()) == 0
        noise = nd.cpu()
    ws_bytes = L.ts_frontend_workspace_bytes(C.byref(d))
    assert ws_bytes >= batch * nf * nm * 4
    wsbuf = torch.full((ws_bytes + 2 * GUARD_BYTES,), 255, dtype=torch.uint8, device="cuda")
    ws = wsbuf[GUARD_BYTES: GUARD_BYTES + ws_bytes]
    fbuf = torch.full((batch * nm + 2 * GUARD_ROWS, pitch), NAN, dtype=BF, device="cuda")
    fbuf[:GUARD_ROWS] = GUARD
    fbuf[GUARD_ROWS + batch * nm:] = GUARD
    feats = fbuf[GUARD_ROWS: GUARD_ROWS + batch * nm]
    fl = torch.full((batch + 2,), -7, dtype=torch.int32, device="cuda")
    fl64 = torch.full((batch + 2,), -7, dtype=torch.int64, device="cuda")
    d.feat_len64 = fl64[1:].data_ptr()
    out = [C.c_int32(-7) for _ in range(4)]
    assert L.ts_frontend_launch_config(C.byref(d), *[C.byref(o) for o in out]) == 0
    cfg = tuple(o.value for o in out)
    st = L.ts_mel_frontend_fwd(C.byref(d), xd.data_ptr(), ld.data_ptr(), feats.data_ptr(), fl[1:].data_ptr(), ws.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert st == 0, f"{case['name']}: ts_mel_frontend_fwd returned {st}"
    assert L.ts_frontend_logmel_ptr(C.byref(d), ws.data_ptr()) == ws.data_ptr()
    what = case["name"]
    assert bool((wsbuf[:GUARD_BYTES] == 255).all()) and bool((wsbuf[GUARD_BYTES + ws_bytes:] == 255).all()), f"{what}: bytes next to the workspace were written"
    assert bool((torch.cat([fbuf[:GUARD_ROWS], fbuf[GUARD_ROWS + batch * nm:]]) == GUARD).all()), f"{what}: a guard row next to the features was written"
    assert fl[0] == -7 and fl[batch + 1] == -7 and fl64[0] == -7 and fl64[batch + 1] == -7
    logmel = ws[: batch * nf * nm * 4].view(torch.float32).view(batch, nf, nm).cpu()
    return cfg, logmel, feats.view(batch, nm, pitch).float().cpu(), fl[1: batch + 1].cpu(), fl64[1: batch + 1].cpu(), noise


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_fused_front_end_matches_the_float64_restatement(case):
    from thunder_speech_amd import _lib
    L = _lib.lib()
    tables = _tables(case)
    keep = []
    query = lambda batch: _host_grid(L, _lib, case, batch, tables, keep)
    batch = _batch_for(case, query)
    x, lens = _wave(case, batch)
    cfg, logmel, feats, fl, fl64, noise = _run_fused(L, _lib, case, batch, tables, x, lens)
    grid, n_groups, lds, di = cfg
    name, hop, n = case["name"], case["hop"], case["n"]
    nf = n // hop + 1
    nwg = (nf + 15) // 16
    print(f"QUERY|{name}|batch={batch}|grid={grid}|n_groups={n_groups}|lds_bytes={lds}|dither_instantiation={di}")
    assert n_groups == batch * nwg and 0 < grid <= n_groups and di == (1 if case["dither"] else 0)
    if case["batch_from_grid"]:
        kind, k, f = case["batch_from_grid"]
        assert n_groups >= f * grid + (k if kind == "groups" else 0), f"{name}: {n_groups} groups on {grid} workgroups"
    win, fb, mw, moff = tables
    r = _restate(x, lens, win, mw, moff, hop, 0.97, masks=case["masks"], noise=noise, dither=case["dither"])
    kind = "dither" if case["dither"] else "eval"
    _report(f"fe-logmel|{kind}", name, (logmel.double().permute(0, 2, 1) - r["logmel"]).abs(), r["e_logmel"])
    assert torch.equal(fl.long(), r["flen"]) and torch.equal(fl64, r["flen"]), f"{name}: feat_len"
    got = feats.double()
    assert not bool(torch.isnan(got).any()), f"{name}: unwritten (NaN) feature elements"
    assert bool((got[:, :, nf:] == 0).all()), f"{name}: columns [n_frames, pitch) are not exactly 0"
    check = ~r["degenerate"][:, :, None].expand(-1, -1, nf)
    err = (got[:, :, :nf] - r["z"]).abs()
    _report(f"fe-features|{kind}", name, torch.where(check, err, torch.zeros_like(err)), r["e_z"])
    zero = ~r["keep"]
    assert bool((got[:, :, :nf][zero] == 0).all()), f"{name}: frames beyond the length or inside a mask rectangle are not exactly 0"
    assert bool(torch.isfinite(got).all())
    for i in case["silent"]:
        assert bool(r["degenerate"][i].all()) and float(r["logmel"][i].max()) == LOG_FLOOR
    assert float(r["z"].abs().max()) > 0.9                                # (two valid frames normalise to -1 and +1)


@pytest.mark.gpu
def test_both_instantiations_walk_at_least_two_passes_and_cross_group_kinds():
    """What the steady-state rows rely on, from the query alone: eval and dither instantiations both get n_groups >= 2 x grid, and in the long-clip
    case the grid is no multiple of the groups per clip, so a workgroup meets edge and interior groups in turn."""
    from thunder_speech_amd import _lib
    L = _lib.lib()
    seen = {}
    for case in CASES:
        if not case["batch_from_grid"]:
            continue
        tables = _tables(case)
        keep = []
        query = lambda batch: _host_grid(L, _lib, case, batch, tables, keep)
        batch = _batch_for(case, query)
        st, (grid, n_groups, lds, di) = query(batch)
        assert st == 0 and n_groups >= 2 * grid
        seen[di] = max(seen.get(di, 0), n_groups // grid)
        if case["name"] == "steady-long":
            assert grid % ((case["n"] // case["hop"] + 1 + 15) // 16) != 0
    assert seen.keys() == {0, 1} and min(seen.values()) >= 2


@pytest.mark.gpu
def test_fused_front_end_refuses_what_it_documents():
    from thunder_speech_amd import _lib
    L = _lib.lib()
    E, U = _lib.TS_EINVAL, _lib.TS_EUNSUPPORTED
    a = torch.zeros(1 << 16, device="cuda").data_ptr()
    base = dict(batch=2, n_samples=6400, n_fft=512, hop=160, win_length=320, n_mels=64, preemph=0.97, n_frames=41, pitch_out=48, window=a, mel_weights=a,
                mel_offsets=a, mel_nnz=100)
    bad = [(dict(window=None), E), (dict(mel_weights=None), E), (dict(mel_offsets=None), E), (dict(batch=0), E), (dict(n_samples=256, n_frames=2), E),
           (dict(hop=0), E), (dict(n_mels=0), E), (dict(n_fft=400), U), (dict(n_fft=1024), U), (dict(win_length=513), E), (dict(win_length=0), E),
           (dict(n_frames=40), E), (dict(pitch_out=44), E), (dict(pitch_out=40), E), (dict(n_masks=-1), E), (dict(n_masks=2), E), (dict(mel_nnz=-1), E),
           (dict(n_mels=257), U), (dict(hop=3000, n_frames=3), U), (dict(mel_nnz=40000), U)]
    out = [C.c_int32(-7) for _ in range(4)]
    for ch, want in bad:
        d = _lib.FrontendDesc(**dict(base, **ch))
        assert L.ts_mel_frontend_fwd(C.byref(d), a, a, a, a, a, None) == want, ch
        assert L.ts_frontend_launch_config(C.byref(d), *[C.byref(o) for o in out]) == want, ch
        assert [o.value for o in out] == [-7] * 4
    d = _lib.FrontendDesc(**base)
    args = [C.byref(d), a, a, a, a, a]
    for i in range(6):
        assert L.ts_mel_frontend_fwd(*[None if j == i else v for j, v in enumerate(args)], None) == E
    assert L.ts_frontend_launch_config(None, *[C.byref(o) for o in out]) == E
    assert L.ts_frontend_launch_config(C.byref(d), None, *[C.byref(o) for o in out[:3]]) == E
    assert L.ts_frontend_workspace_bytes(None) == E
    for ch in (dict(batch=0), dict(n_frames=0), dict(n_mels=0)):
        assert L.ts_frontend_workspace_bytes(C.byref(_lib.FrontendDesc(**dict(base, **ch)))) == E
    assert L.ts_frontend_launch_config(C.byref(d), *[C.byref(o) for o in out]) == 0 and out[1].value == 2 * 3 and out[3].value == 0


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the stage kernels, each against float64 with the plain-sum bound of its loop
# ---------------------------------------------------------------------------------------------------------------------
def _dev_out(shape):
    n = int(np.prod(shape))
    buf = torch.full((n + 128,), NAN, device="cuda")
    buf[:64] = GUARD
    buf[64 + n:] = GUARD
    return buf, buf[64: 64 + n].view(shape)


def _flat_guards_ok(buf, n, what):
    assert bool((buf[:64] == GUARD).all()) and bool((buf[64 + n:] == GUARD).all()), f"{what}: the guard next to the output was written"


@pytest.mark.gpu
@pytest.mark.parametrize("batch,n,coeff", [(3, 1001, 0.97), (1, 1, 0.5), (2, 257, 0.0)])
def test_stage_preemph(batch, n, coeff):
    """y = x - c x[-1]: a product and a difference, bound u (|c x[-1]| + |y|); sample 0 is copied, bound 0"""
    from thunder_speech_amd import _lib
    L = _lib.lib()
    x = torch.randn(batch, n, generator=torch.Generator().manual_seed(n))
    xd = x.cuda()
    buf, y = _dev_out((batch, n))
    assert L.ts_fe_preemph(xd.data_ptr(), y.data_ptr(), batch, n, coeff, _stream()) == 0
    torch.cuda.synchronize()
    c = float(np.float32(coeff))
    ref = x.double().clone()
    ref[:, 1:] = x.double()[:, 1:] - c * x.double()[:, :-1]
    bound = torch.zeros_like(ref)
    bound[:, 1:] = U32 * ((c * x.double()[:, :-1]).abs() + ref[:, 1:].abs())
    _report("fe-stage|preemph", f"n={n} coeff={coeff}", (y.double().cpu() - ref).abs(), bound)
    _flat_guards_ok(buf, batch * n, "preemph")
    assert L.ts_fe_preemph(None, y.data_ptr(), batch, n, coeff, None) == _lib.TS_EINVAL and L.ts_fe_preemph(xd.data_ptr(), y.data_ptr(), 0, n, coeff, None) == -1
    assert L.ts_fe_preemph(xd.data_ptr(), None, batch, n, coeff, None) == -1 and L.ts_fe_preemph(xd.data_ptr(), y.data_ptr(), batch, 0, coeff, None) == -1


def _philox_words(seed, stream_id, counter):
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


@pytest.mark.gpu
@pytest.mark.parametrize("batch,n,dither,seed", [(3, 1001, 1e-5, 7), (2, 4096, 1.0, 0xFEDCBA9876543210), (1, 1, 0.5, 1 << 63)])
def test_stage_dither(batch, n, dither, seed):
    """y = x + d N(0, 1): sample k of clip b draws philox(seed, stream 1, (b << 32) | (k >> 1)), Box-Muller r = sqrt(-2 ln u1), (n0, n1) = r (cos, sin)(2 pi u2)
    with u1 = ((w0 >> 8) + 1) 2^-24, u2 = (w1 >> 8) 2^-24 (both exact in f32).  Bound: L = -2 ln u1 through the fast logf, dL = 2 (4 u |ln u1| + 2 u);
    r = sqrt L (v_sqrt_f32, 1 ulp): dr = min(dL / r, sqrt dL) + 2 u r; sincospif 4 u; the product u: dn = dr + 4 u r + u |n|; then the product with d and
    the add: u (|d n| + |y|) + |d| dn."""
    from thunder_speech_amd import _lib
    L = _lib.lib()
    x = torch.randn(batch, n, generator=torch.Generator().manual_seed(n))
    xd = x.cuda()
    buf, y = _dev_out((batch, n))
    assert L.ts_fe_dither(xd.data_ptr(), y.data_ptr(), batch, n, dither, seed, _stream()) == 0
    torch.cuda.synchronize()
    pairs = (n + 1) // 2
    counter = (np.arange(batch, dtype=np.uint64)[:, None] << np.uint64(32)) | np.arange(pairs, dtype=np.uint64)[None, :]
    w0, w1, _, _ = _philox_words(seed, 1, counter)
    u1 = ((w0 >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u2 = (w1 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    lnu = np.log(u1)
    big_l = -2.0 * lnu
    r = np.sqrt(big_l)
    d_l = 2 * (4 * U32 * np.abs(lnu) + 2 * U32)
    d_r = np.minimum(d_l / np.maximum(r, 1e-300), np.sqrt(d_l)) + 2 * U32 * r
    noise = np.stack([r * np.cos(2 * np.pi * u2), r * np.sin(2 * np.pi * u2)], -1).reshape(batch, 2 * pairs)[:, :n]
    d_n = np.repeat(d_r + 4 * U32 * r, 2, axis=-1).reshape(batch, 2 * pairs)[:, :n] + U32 * np.abs(noise)
    d = float(np.float32(dither))
    ref = x.double() + d * torch.from_numpy(noise)
    bound = U32 * ((d * torch.from_numpy(noise)).abs() + ref.abs()) + abs(d) * torch.from_numpy(d_n)
    _report("fe-stage|dither", f"n={n} dither={dither}", (y.double().cpu() - ref).abs(), bound)
    _flat_guards_ok(buf, batch * n, "dither")
    if n >= 4096:
        got = (y.double().cpu() - x.double()) / d
        assert abs(float(got.mean())) < 0.05 and abs(float(got.std()) - 1.0) < 0.05
    assert L.ts_fe_dither(None, y.data_ptr(), batch, n, dither, seed, None) == -1 and L.ts_fe_dither(xd.data_ptr(), y.data_ptr(), batch, 0, dither, seed, None) == -1


def _dft_reference(x, win, tw, n_fft, hop):
    """float64 (re, im, bound per component) [B][n_freq][frames] of the direct DFT over the f32 twiddle table the device holds"""
    b, n = x.shape
    half = n_fft // 2
    pad = F.pad(x.double()[:, None, :], (half, half), mode="reflect")[:, 0]
    frames = pad.unfold(-1, n_fft, hop) * win.double()                                                   # [B][F][n_fft]
    n_freq = half + 1
    idx = (torch.arange(n_freq)[:, None] * torch.arange(n_fft)[None, :]) % n_fft                         # [n_freq][n_fft]
    cos, sin = tw[:, 0].double()[idx], tw[:, 1].double()[idx]
    re = torch.einsum("bfj,kj->bkf", frames, cos)
    im = -torch.einsum("bfj,kj->bkf", frames, sin)
    # every term |frame| |tw| <= |frame| through at most n_fft roundings, and the product x win rounded once
    bound = ((n_fft + 1) * U32 / (1 - (n_fft + 1) * U32)) * frames.abs().sum(-1)[:, None, :].expand_as(re)
    return re, im, bound


STFT_SHAPES = [(2, 2, 1, 7), (400, 160, 2, 1000), (512, 160, 3, 1700), (1024, 256, 1, 3000), (64, 100, 2, 333)]      # n_fft, hop, batch, n


@pytest.mark.gpu
@pytest.mark.parametrize("n_fft,hop,batch,n", STFT_SHAPES, ids=[f"nfft{a}-hop{b}" for a, b, _, _ in STFT_SHAPES])
def test_stage_stft_and_power_spectrum(n_fft, hop, batch, n):
    """ts_fe_stft (re, im) and ts_fe_power_spectrum: per component (n_fft + 1) u sum |frame| (the plain-sum bound of the DFT loop, plus the rounding of
    x win); the power re^2 + im^2 on top: 2 (|re| + |im|) e + 2 e^2 + 3 u P."""
    from thunder_speech_amd import _lib
    L = _lib.lib()
    g = torch.Generator().manual_seed(n_fft)
    x = torch.randn(batch, n, generator=g)
    win = torch.rand(n_fft, generator=g) + 0.1
    ang = 2 * math.pi * torch.arange(n_fft, dtype=torch.float64) / n_fft
    tw = torch.stack([torch.cos(ang), torch.sin(ang)], -1).float()
    xd, wd, twd = x.cuda(), win.cuda(), tw.cuda()
    frames = n // hop + 1
    n_freq = n_fft // 2 + 1
    re, im, e = _dft_reference(x, win, tw, n_fft, hop)
    assert re.shape == (batch, n_freq, frames)
    buf, out = _dev_out((batch, n_freq, frames, 2))
    assert L.ts_fe_stft(xd.data_ptr(), wd.data_ptr(), twd.data_ptr(), out.data_ptr(), batch, n, n_fft, hop, _stream()) == 0
    torch.cuda.synchronize()
    got = out.double().cpu()
    what = f"n_fft={n_fft} hop={hop} n={n}"
    _report("fe-stage|stft-re", what, (got[..., 0] - re).abs(), e)
    _report("fe-stage|stft-im", what, (got[..., 1] - im).abs(), e)
    _flat_guards_ok(buf, out.numel(), "stft")
    buf, out = _dev_out((batch, n_freq, frames))
    assert L.ts_fe_power_spectrum(xd.data_ptr(), wd.data_ptr(), twd.data_ptr(), out.data_ptr(), batch, n, n_fft, hop, _stream()) == 0
    torch.cuda.synchronize()
    p = re * re + im * im
    bound = 2 * (re.abs() + im.abs()) * e + 2 * e * e
    bound = bound + 3 * U32 * (p + bound)
    _report("fe-stage|power", what, (out.double().cpu() - p).abs(), bound)
    _flat_guards_ok(buf, out.numel(), "power spectrum")
    # reflect padding needs n_fft / 2 < n
    for fn in (L.ts_fe_stft, L.ts_fe_power_spectrum):
        assert fn(xd.data_ptr(), wd.data_ptr(), twd.data_ptr(), out.data_ptr(), batch, n_fft // 2, n_fft, hop, None) == _lib.TS_EINVAL
        assert fn(xd.data_ptr(), wd.data_ptr(), twd.data_ptr(), out.data_ptr(), batch, n, 1, hop, None) == _lib.TS_EINVAL
        assert fn(xd.data_ptr(), wd.data_ptr(), twd.data_ptr(), out.data_ptr(), batch, n, n_fft, 0, None) == _lib.TS_EINVAL
        assert fn(xd.data_ptr(), None, twd.data_ptr(), out.data_ptr(), batch, n, n_fft, hop, None) == _lib.TS_EINVAL


@pytest.mark.gpu
@pytest.mark.parametrize("log_scale", [0, 1])
@pytest.mark.parametrize("n_freq,n_mels,t", [(257, 64, 41), (2, 1, 1), (201, 13, 70)])
def test_stage_mel(n_freq, n_mels, t, log_scale):
    """acc += w x over n_freq terms: n_freq u sum |w x|; with the log: the add of the floor (u v), -log1p(-d / v), and the fast logf (4 u |log v| + 2 u)"""
    from thunder_speech_amd import _lib
    L = _lib.lib()
    g = torch.Generator().manual_seed(n_freq + t)
    x = torch.rand(2, n_freq, t, generator=g) * 3.0
    x[0, :, 0] = 0.0                                                       # a silent frame: log(2^-24)
    fb = torch.rand(n_mels, n_freq, generator=g) * (torch.rand(n_mels, n_freq, generator=g) < 0.3)
    xd, fd = x.cuda(), fb.cuda()
    buf, out = _dev_out((2, n_mels, t))
    assert L.ts_fe_mel(xd.data_ptr(), fd.data_ptr(), out.data_ptr(), 2, n_freq, n_mels, t, log_scale, _stream()) == 0
    torch.cuda.synchronize()
    acc = torch.einsum("mf,bft->bmt", fb.double(), x.double())
    e = (n_freq * U32 / (1 - n_freq * U32)) * acc                          # every product is >= 0: sum |w x| = acc
    if log_scale:
        v = acc + FLOOR
        e = e + U32 * v
        assert bool((e <= v / 4).all())
        ref = torch.log(v)
        e = -torch.log1p(-e / v) + 4 * U32 * ref.abs() + 2 * U32
    else:
        ref = acc
    _report(f"fe-stage|mel-log{log_scale}", f"n_freq={n_freq} n_mels={n_mels} t={t}", (out.double().cpu() - ref).abs(), e)
    _flat_guards_ok(buf, out.numel(), "mel")
    assert L.ts_fe_mel(xd.data_ptr(), fd.data_ptr(), out.data_ptr(), 2, 0, n_mels, t, log_scale, None) == _lib.TS_EINVAL
    assert L.ts_fe_mel(xd.data_ptr(), None, out.data_ptr(), 2, n_freq, n_mels, t, log_scale, None) == _lib.TS_EINVAL


@pytest.mark.gpu
@pytest.mark.parametrize("features,t,lens", [(5, 70, [0, 1, 70, 33]), (1, 1, [1, 0]), (3, 200, [200, 199, 65, -4, 300])])
def test_stage_normalize(features, t, lens):
    """The sums run in f64 (their error is below 2^-50 of the absolute sums: ignored next to u).  mean rounded to f32 (u |mean|), the difference (u), the f32
    square root, the add of the guard, the reciprocal (v_rcp_f32, 2 u) and the product: 6 u relative on the scale factor.
    Length 0: the mean is 0 / 0 and every frame is masked: the output is exactly 0, no NaN."""
    from thunder_speech_amd import _lib
    L = _lib.lib()
    b = len(lens)
    g = torch.Generator().manual_seed(t)
    x = torch.randn(b, features, t, generator=g) * 3.0 - 7.0
    xd, ld = x.cuda(), torch.tensor(lens, dtype=torch.int32).cuda()
    guard = 1e-5
    buf, out = _dev_out((b, features, t))
    assert L.ts_fe_normalize(xd.data_ptr(), ld.data_ptr(), out.data_ptr(), b, features, t, guard, _stream()) == 0
    torch.cuda.synchronize()
    n = torch.tensor(lens).clamp(0, t)
    valid = (torch.arange(t)[None, :] < n[:, None])[:, None, :]
    nn = n.double()[:, None, None].clamp_min(1)
    xz = x.double() * valid
    mean = xz.sum(-1, keepdim=True) / nn
    var = ((((x.double() - mean) ** 2) * valid).sum(-1, keepdim=True) + (t - nn) * mean * mean) / nn
    inv = 1.0 / (var.sqrt() + float(np.float32(guard)))
    diff = x.double() - mean
    ref = diff * inv * valid
    e = (U32 * mean.abs() + U32 * (diff.abs() + U32 * mean.abs())) * inv * (1 + 6 * U32) + 6 * U32 * ref.abs() + U32 * ref.abs()
    e = e * valid
    _report("fe-stage|normalize", f"features={features} t={t} lens={lens}", (out.double().cpu() - ref).abs(), e)
    _flat_guards_ok(buf, out.numel(), "normalize")
    assert L.ts_fe_normalize(xd.data_ptr(), None, out.data_ptr(), b, features, t, guard, None) == _lib.TS_EINVAL
    assert L.ts_fe_normalize(xd.data_ptr(), ld.data_ptr(), out.data_ptr(), b, features, 0, guard, None) == _lib.TS_EINVAL
