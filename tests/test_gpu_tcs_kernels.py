"""Every instantiation behind ts_tcs_subblock_fwd (csrc/tcs_kernel.hip, csrc/tcs_split.hip, csrc/pw_logits.hip), launched through the C ABI, asserted BY
NAME through ts_tcs_last_launch and compared per element with a plain float64 restatement of the sub-block on the CPU (F.conv1d and einsum in float64;
nothing of thunder_speech_amd or oracle).  tests/test_gpu_tcs.py compares the same entry point against the fp32 oracle with one bound per tensor and
cannot tell which kernel answered; here a row of CASES names the kernel it must reach, and a row that reaches another one fails.

The restatement reads the operands the device holds: x and the residual input rounded to bf16, the depthwise taps rounded to bf16, the folded weights
bf16(pw x scale) and bf16(res_w x res_scale) (scale = gamma / sqrt(var + 1e-3), formed in f32 as plan.make_tcs_layer forms it), the f32 shift.  Steps:
mask x at its length; depthwise convolution; re-mask at the output length; pointwise product; + the 1x1 product of the masked residual input taken at
frames t x res_stride; + shift; squeeze-excite form relu(gate x se_y + result) where given; ReLU when set; 0 beyond the output length with
TS_TCS_OUT_ZERO_TAIL, otherwise the restatement's own values there (quirk A2: relu(shift + residual part)).
test_reference_restatement_matches_the_fp32_oracle (no gpu mark) pins it against oracle.tcs.block_forward(emulate_bf16=False) on operands both read alike.

Bound, per element, from the roundings between operands and store (u16 = 2^-8, the unit roundoff of bf16 under round-to-nearest-even: 8 significand
bits, half an ulp of a value in [2^e, 2^(e+1)) is 2^(e-8) -- every conversion in the three files is v_cvt_pk_bf16_f32 or the plain cast; u32 = 2^-24):
  1. depthwise result.  Products of two bf16 values are exact in f32; a lane's v_mfma_f32_4x4x4_16b_bf16 chain adds n_dw = 4 x dw_ksteps of them
     (the zeros of the Toeplitz rows included) in f32:            e0 = n_dw u32 (|taps| * |x|)[t]           (the convolution of the absolute values)
     and the sum is rounded to bf16, as the MFMA operand:         E_mid = e0 + u16 (|mid| + e0)
     A pointwise-only layer stages its input unchanged:           E_mid = 0
  2. pointwise + residual products, f32 accumulation over n = c_in_pad64 + c_res_pad64 + 4 terms (the padded channels, the shift as the initial
     accumulator, the three joins of pw_logits' four partial sums):
                                                                  E_pre = |wf| E_mid + n u32 P,   P = |wf| (|mid| + E_mid) + |rwf| |x_res| + |shift|
  3. store.  f32: E = E_pre.  bf16 (ReLU is 1-Lipschitz):          E = E_pre + u16 (|ref| + E_pre)
     squeeze-excite form: the result is rounded to bf16 first      E_r = E_pre + u16 (|pre| + E_pre)
     one fmaf(se_y, gate, result) in f32                           E_v = E_r + u32 (|gate se_y + pre| + E_r)
     ReLU, bf16 store                                              E = E_v + u16 (|ref| + E_v)
  Frames zeroed by TS_TCS_OUT_ZERO_TAIL have bound 0: they must be exactly 0.
Per-tile statistics (ts_tcs_desc.stats) are sums of the f32 accumulators a = s / (1 + d), |d| <= u16, s the stored bf16 value (cases with relu = 0):
  sum:          rho sum |s| + (n + 1) u32 (1 + rho) sum |s|,            rho = u16 / (1 - u16), n = frames of the tile (f32 adds, one shuffle step)
  sum of squares: rho (2 + rho) sum s^2 + (n + 1) u32 (1 + rho)^2 sum s^2
compared against float64 sums of the stored values.  Nothing here is fitted to measured ratios (profiles/tcs_kernel_checks.md has those).

Conventions of every case: the return code and the launch record are asserted; the output is a view inside a larger NaN-filled buffer whose guard rows
(7.0) before and after it must come back bit for bit; masked inputs hold random values from their length to t and NaN from t to the pitch; tail-zero
inputs are built by hand as thunder_speech_amd/tensors.py builds them (0 from the length to the pitch, TS_GUARD_BYTES of zeros on both sides);
device tensors live to the end of the test (_keep); every check prints `RATIO|kind|error / bound` before it asserts; no element is left out."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

NAN = float("nan")
BF = torch.bfloat16
GUARD = 7.0
GUARD_ROWS = 32
U16 = 2.0 ** -8
U32 = 2.0 ** -24
BN_EPS = 1e-3
KC = 64

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "thunder_speech_amd", "csrc")


# ---------------------------------------------------------------------------------------------------------------------
# the instantiations, as the launch record names them
# ---------------------------------------------------------------------------------------------------------------------
def G(tt, nt, stride, dw, f32, tlds, tz, xj, npass):
    return ("generic", tt, nt, stride, int(dw), int(f32), int(tlds), int(tz), xj, npass)


def S(npass, xj, wm, dil, se):
    return ("split", npass, xj, wm, dil, int(se))


LOGITS = ("logits",)


def _case(name, expect, cin, cout, k, t, lens, **kw):
    d = dict(name=name, expect=expect, cin=cin, cout=cout, k=k, t=t, lens=lens, stride=1, dil=1, cres=0, res_stride=1, relu=True, mode="masked",
             zero_tail=None, refuse=None, f32=False, se=False, stats=False, phase=False, xcd=None, wrap=False, tile_frames=None, tt_logits=None)
    d.update(kw)
    if d["zero_tail"] is None:
        d["zero_tail"] = d["mode"] == "tz"
    return d


def _cycle(vals, n):
    return [vals[i % len(vals)] for i in range(n)]


TZ = dict(mode="tz")
CASES = [
    # ---- straight-line tail-zero depthwise kernels: tail-zero tensors, the split kernel refused (no raw taps / an output pitch below its tiling)
    _case("tz-128-np1", G(128, 2, 1, 1, 0, 1, 1, 3, 1), 64, 64, 5, 257, [257, 129, 1], refuse="taps_raw", **TZ),
    _case("tz-128-np2", G(128, 2, 1, 1, 0, 1, 1, 3, 2), 64, 40, 11, 200, [200, 199, 127], refuse="pitch", **TZ),
    _case("tz-128-np3-res", G(128, 2, 1, 1, 0, 1, 1, 3, 3), 128, 256, 33, 130, [130, 128, 127], refuse="taps_raw", cres=64, **TZ),
    _case("tz-128-np4", G(128, 2, 1, 1, 0, 1, 1, 3, 4), 64, 128, 39, 129, [129, 128, 64], refuse="pitch", relu=False, **TZ),
    _case("tz-64-np3", G(64, 4, 1, 1, 0, 1, 1, 2, 3), 64, 288, 25, 130, [130, 65, 63], refuse="taps_raw", **TZ),
    _case("tz-64-np5", G(64, 4, 1, 1, 0, 1, 1, 2, 5), 128, 512, 51, 100, [100, 64, 1], refuse="pitch", **TZ),
    _case("tz-64-np6-res", G(64, 4, 1, 1, 0, 1, 1, 3, 6), 64, 320, 63, 65, [65, 64], refuse="taps_raw", cres=128, **TZ),
    _case("tz-64-np7-640", G(64, 4, 1, 1, 0, 1, 1, 3, 7), 64, 640, 75, 129, [129, 127, 2], refuse="pitch", **TZ),
    _case("tz-64-k87-dil2", G(64, 4, 1, 1, 0, 0, 1, 4, 15), 64, 512, 87, 131, [131, 130, 66], dil=2, **TZ),       # phase-split form not offered
    _case("tz-128-stride2", G(128, 2, 2, 1, 0, 1, 1, 5, 4), 64, 256, 33, 515, [515, 257, 255], stride=2, **TZ),
    # ---- depthwise kernels with run-time geometry: masked caller tensors; taps in LDS, or from global memory (dw_ksteps > 24)
    _case("any-64-lds", G(64, 4, 1, 1, 0, 1, 0, 0, 0), 24, 300, 13, 70, [70, 65, 1], dil=3, relu=False),
    _case("any-128-lds-res", G(128, 2, 1, 1, 0, 1, 0, 0, 0), 80, 40, 11, 130, [130, 129, 127], cres=24),
    _case("any-64-s2-lds-res2", G(64, 4, 2, 1, 0, 1, 0, 0, 0), 24, 320, 9, 131, [131, 130, 3], stride=2, cres=80, res_stride=2),
    _case("any-128-s2-lds", G(128, 2, 2, 1, 0, 1, 0, 0, 0), 80, 29, 33, 259, [259, 258, 1], stride=2),
    _case("any-64-global", G(64, 4, 1, 1, 0, 0, 0, 0, 0), 24, 264, 101, 66, [66, 64, 33]),
    _case("any-128-global", G(128, 2, 1, 1, 0, 0, 0, 0, 0), 80, 40, 35, 129, [129, 128], dil=3, relu=False),
    _case("any-64-s2-global", G(64, 4, 2, 1, 0, 0, 0, 0, 0), 64, 512, 101, 131, [131, 129], stride=2),
    # ---- pointwise only, generic kernel
    _case("pw-tz-64", G(64, 4, 1, 0, 0, 0, 1, 0, 0), 64, 320, 1, 100, [100, 65, 1], refuse="pitch", **TZ),
    _case("pw-tz-128", G(128, 2, 1, 0, 0, 0, 1, 0, 0), 128, 40, 1, 200, [200, 129, 127], refuse="pitch", **TZ),
    _case("pw-tz-128-res", G(128, 2, 1, 0, 0, 0, 1, 0, 0), 64, 256, 1, 130, [130, 128, 1], cres=64, **TZ),     # a residual: no split launch
    _case("pw-masked-64x512-stats", G(64, 4, 1, 0, 0, 0, 0, 0, 0), 24, 300, 1, 70, [70, 65, 1], stats=True, relu=False, tile_frames=64),
    _case("pw-masked-128-stats", G(128, 2, 1, 0, 0, 0, 0, 0, 0), 24, 40, 1, 513, _cycle([513, 512, 385, 129, 1], 64), stats=True, relu=False,
          tile_frames=128),
    _case("pw-masked-64x256-stats", G(64, 2, 1, 0, 0, 0, 0, 0, 0), 80, 29, 1, 130, [130, 129, 63], stats=True, relu=False, tile_frames=64),
    _case("pw-masked-64x256-res", G(64, 2, 1, 0, 0, 0, 0, 0, 0), 80, 40, 1, 65, [65, 64, 1], cres=24, tile_frames=64),
    _case("pw-s2-64", G(64, 4, 2, 0, 0, 0, 0, 0, 0), 24, 300, 1, 131, [131, 130, 1], stride=2),
    _case("pw-s2-128", G(128, 2, 2, 0, 0, 0, 0, 0, 0), 80, 40, 1, 259, [259, 257, 2], stride=2, relu=False),
    _case("pw-f32-generic-cin64", G(128, 2, 1, 0, 1, 0, 0, 0, 0), 64, 29, 1, 130, [130, 129, 1], f32=True, relu=False),
    _case("pw-f32-generic-cout40-zero-tail", G(128, 2, 1, 0, 1, 0, 0, 0, 0), 128, 40, 1, 129, [129, 128], f32=True, relu=False, zero_tail=True),
    # ---- pw_logits
    _case("logits-29", LOGITS, 128, 29, 1, 200, [200, 97, 1], f32=True, relu=False, tt_logits=96),
    _case("logits-32-zero-tail", LOGITS, 256, 32, 1, 97, [97, 96, 95], f32=True, relu=False, zero_tail=True, tt_logits=96),
    _case("logits-29-128-frame-tiles", LOGITS, 128, 29, 1, 380, _cycle([380, 379, 257, 129, 1], 129), f32=True, relu=False, tt_logits=128),
    # ---- split kernel
    _case("split-np3-wm2-res1", S(3, 4, 2, 1, 0), 64, 256, 33, 385, [385, 193, 191], cres=64, **TZ),
    _case("split-np4-wm2-res2", S(4, 4, 2, 1, 0), 128, 40, 39, 200, [200, 192, 1], cres=128, **TZ),
    _case("split-np2-wm2", S(2, 4, 2, 1, 0), 64, 128, 17, 193, [193, 192, 100], relu=False, **TZ),
    _case("split-pw-wm2-keeps-tail", S(2, 4, 2, 1, 0), 128, 256, 1, 200, [200, 191, 1], mode="tz", zero_tail=False),
    _case("split-np5-res3", S(5, 3, 1, 1, 0), 64, 512, 51, 97, [97, 96, 95], cres=192, xcd=0, **TZ),
    _case("split-np6", S(6, 3, 1, 1, 0), 128, 320, 63, 200, [200, 97, 1], **TZ),
    _case("split-np7-640-res2", S(7, 3, 1, 1, 0), 64, 640, 75, 100, [100, 96], cres=128, **TZ),
    _case("split-np2-wraps", S(2, 2, 1, 1, 0), 64, 512, 11, 97, _cycle([97, 96, 95, 1], 130), xcd=1, wrap=True, **TZ),
    _case("split-pw-640", S(2, 2, 1, 1, 0), 64, 640, 1, 100, [100, 97, 1], **TZ),
    _case("split-np3-xcd", S(3, 3, 1, 1, 0), 64, 384, 25, 193, [193, 97, 96, 1, 192, 95, 2, 193], xcd=1, **TZ),   # 8 clips x 3 time tiles: a grid of 24
    _case("split-np4", S(4, 3, 1, 1, 0), 64, 288, 41, 97, [97, 1], **TZ),
    _case("split-k87-phase", S(8, 5, 1, 2, 0), 64, 512, 87, 195, [195, 194, 97, 2], dil=2, phase=True, **TZ),
    _case("split-se-wm1", S(2, 2, 1, 1, 1), 64, 640, 1, 100, [100, 97, 50], se=True, **TZ),
    _case("split-se-wm2", S(2, 4, 2, 1, 1), 128, 256, 1, 200, [200, 193, 1], se=True, relu=False, **TZ),
]
# TS_ANY(128, 2, 2, true, false, false): stride 2 on 128-frame tiles with the taps read from global memory.  The dispatcher reads taps from global
# memory only for dw_ksteps > 24 and refuses staged rows beyond 320 frames; on 128-frame tiles at stride 2 a row holds
# woff + 3 x 32 x 2 + 4 x (7 x 2 + dw_ksteps) >= 356 frames for dw_ksteps >= 27, so ts_tcs_subblock_fwd never launches it
# (test_the_unreachable_instantiation_is_refused_by_the_dispatcher; tests/test_capi_host.py holds the same descriptor)
UNREACHABLE = {G(128, 2, 2, 1, 0, 0, 0, 0, 0)}


# ---------------------------------------------------------------------------------------------------------------------
# operands and the float64 restatement
# ---------------------------------------------------------------------------------------------------------------------
def _bf(x):
    return x.float().to(BF).float()


def _mask(lens, t):
    """[B][1][t] float64: frames < clamp(len, 0, t)"""
    return (torch.arange(t)[None, :] < lens.long().clamp(0, t)[:, None]).double()[:, None, :]


def _pad(k, dil):
    return dil * (k - 1) // 2


def _conv_len(lens, k, stride, pad, dil):
    num = lens.long() + 2 * pad - dil * (k - 1) - 1
    return torch.where(num < 0, torch.zeros_like(num), torch.div(num, stride, rounding_mode="floor") + 1)


def _bn(g, c, pow2):
    """(gamma, beta, running_mean, running_var).  pow2: the folded scale is an exact power of two, so that bf16 weights x scale stay bf16"""
    if pow2:
        gamma = 2.0 ** torch.randint(-1, 2, (c,), generator=g).float()
        var = torch.tensor(1.0) - torch.tensor(BN_EPS)
        for cand in (var, torch.nextafter(var, torch.tensor(2.0)), torch.nextafter(var, torch.tensor(0.0))):
            if float(torch.sqrt(cand + BN_EPS)) == 1.0:
                var = cand
                break
        else:
            raise AssertionError("no f32 variance with sqrt(var + eps) == 1")
        var = var.expand(c).clone()
    else:
        gamma = 1.0 + 0.1 * torch.randn(c, generator=g)
        var = 0.5 + torch.rand(c, generator=g)
    return [gamma, 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g), var]


def _fold(bn):
    scale = bn[0] / torch.sqrt(bn[3] + BN_EPS)                     # f32, the expression of plan.fold_bn
    return scale, bn[1] - bn[2] * scale


def _operands(case, seed, pow2=False):
    """What the device holds, as f32 tensors on the CPU (bf16 operands already rounded), and the reference-layout parameters they come from."""
    g = torch.Generator().manual_seed(seed)
    b, cin, cout, k, t = len(case["lens"]), case["cin"], case["cout"], case["k"], case["t"]
    op = dict(case)
    op["lens_t"] = torch.tensor(case["lens"])
    op["x"] = _bf(torch.randn(b, cin, t, generator=g))
    dw = k > 1
    op["dw_w"] = _bf(torch.randn(cin, 1, k, generator=g) * (1.5 / k ** 0.5)) if dw else None
    pw = torch.randn(cout, cin, generator=g) / cin ** 0.5
    op["pw_w"] = _bf(pw) if pow2 else pw
    op["bn"] = _bn(g, cout, pow2)
    scale, shift = _fold(op["bn"])
    op["wf"] = _bf(op["pw_w"] * scale[:, None])
    if case["cres"]:
        cres = case["cres"]
        op["xres"] = _bf(torch.randn(b, cres, t, generator=g))
        rw = torch.randn(cout, cres, generator=g) / cres ** 0.5
        op["res_w"] = _bf(rw) if pow2 else rw
        op["res_bn"] = _bn(g, cout, pow2)
        rs, rsh = _fold(op["res_bn"])
        op["rwf"] = _bf(op["res_w"] * rs[:, None])
        shift = shift + rsh
    op["shift"] = shift
    if case["se"]:
        t_out = t
        op["se_y"] = _bf(torch.randn(b, cout, t_out, generator=g)) * _mask(op["lens_t"], t_out).float()
        op["gate"] = torch.sigmoid(torch.randn(b, cout, generator=g))
    return op


def _reference(op, n_dw):
    """float64: (ref, bound, len_out).  n_dw: products a depthwise output accumulates (4 x dw_ksteps of the launch)"""
    x = op["x"].double()
    b, cin, t = x.shape
    lens, stride, dil, k = op["lens_t"], op["stride"], op["dil"], op["k"]
    xm = x * _mask(lens, t)
    wf = op["wf"].double()
    if op["dw_w"] is not None:
        w, pad = op["dw_w"].double(), _pad(k, dil)
        mid = F.conv1d(xm, w, None, stride, pad, dil, cin)
        amid = F.conv1d(xm.abs(), w.abs(), None, stride, pad, dil, cin)
        len_out = _conv_len(lens, k, stride, pad, dil)
        m = _mask(len_out, mid.shape[-1])
        mid, amid = mid * m, amid * m
        e0 = n_dw * U32 * amid
        e_mid = e0 + U16 * (mid.abs() + e0)
    else:
        mid = xm[:, :, ::stride]
        len_out = _conv_len(lens, 1, stride, 0, 1)
        e_mid = torch.zeros_like(mid)
    t_out = mid.shape[-1]
    pre = torch.einsum("oc,bct->bot", wf, mid)
    prod = torch.einsum("oc,bct->bot", wf.abs(), mid.abs() + e_mid)
    e_pre = torch.einsum("oc,bct->bot", wf.abs(), e_mid)
    n_terms = (cin + KC - 1) // KC * KC + 4
    if op["cres"]:
        xr = op["xres"].double()
        xr = (xr * _mask(lens, xr.shape[-1]))[:, :, ::op["res_stride"]]
        xr = F.pad(xr, (0, max(0, t_out - xr.shape[-1])))[:, :, :t_out]
        rwf = op["rwf"].double()
        pre = pre + torch.einsum("oc,bct->bot", rwf, xr)
        prod = prod + torch.einsum("oc,bct->bot", rwf.abs(), xr.abs())
        n_terms += (op["cres"] + KC - 1) // KC * KC
    shift = op["shift"].double()[None, :, None]
    pre = pre + shift
    e_pre = e_pre + n_terms * U32 * (prod + shift.abs())
    if op["se"]:
        v = op["gate"].double()[:, :, None] * op["se_y"].double() + pre
        ref = torch.relu(v)
        e_r = e_pre + U16 * (pre.abs() + e_pre)
        e_v = e_r + U32 * (v.abs() + e_r)
        bound = e_v + U16 * (ref.abs() + e_v)
    else:
        ref = torch.relu(pre) if op["relu"] else pre
        bound = e_pre if op["f32"] else e_pre + U16 * (ref.abs() + e_pre)
    if op["zero_tail"]:
        m = _mask(len_out, t_out)
        ref, bound = ref * m, bound * m
    return ref, bound, len_out


def _report(kind, what, err, bound):
    ratio = float((err / bound.clamp_min(1e-300)).max()) if bool((bound > 0).any()) else 0.0
    worst = int((err - bound).argmax())
    print(f"RATIO|{kind}|{ratio:.3e}|{what}")
    assert not bool(torch.isnan(err).any()), f"{what}: unwritten (NaN) elements"
    assert bool((err <= bound).all()), (f"{what}: error {float(err.flatten()[worst]):.3e} > bound {float(bound.flatten()[worst]):.3e} at flat index {worst} "
                                        f"(largest error / bound {ratio:.3e})")


# ---------------------------------------------------------------------------------------------------------------------
# CPU tests: the restatement against the fp32 oracle, the case table against the sources
# ---------------------------------------------------------------------------------------------------------------------
PIN_SHAPES = [          # cin, cout, k, stride, dil, t, lens, residual
    (24, 40, 11, 1, 1, 70, [70, 33, 1], True),
    (80, 29, 33, 2, 1, 131, [131, 130, 64], True),
    (24, 40, 13, 1, 3, 45, [45, 30], False),
    (64, 64, 87, 1, 2, 131, [131, 66], False),
    (80, 40, 1, 1, 1, 65, [65, 64, 1], False),
]


@pytest.mark.parametrize("cin,cout,k,stride,dil,t,lens,res", PIN_SHAPES)
def test_reference_restatement_matches_the_fp32_oracle(cin, cout, k, stride, dil, t, lens, res):
    """oracle.tcs.block_forward(emulate_bf16=False) on operands both read alike: bf16 taps and weights, BatchNorm scales that are exact powers of two
    (bf16(pw x scale) = pw x scale), so the two differ by f32 rounding only: (K + c_in + c_res + 8) x 2^-23 x the absolute sum of every product and of
    the BatchNorm terms.  The oracle keeps its own values beyond the length (quirk A2), and so does the restatement without the zero-tail flag."""
    from oracle import tcs as otcs
    case = _case("pin", None, cin, cout, k, t, lens, stride=stride, dil=dil, cres=cin if res else 0, res_stride=stride, zero_tail=False)
    op = _operands(case, seed=11 * k + cin, pow2=True)
    if res:
        op["xres"] = op["x"]                                       # a block's residual branch reads the block's input
    ref, _, len_out = _reference(op, 0)
    spec = otcs.BlockSpec(cin, cout, repeat=1, kernel=k, stride=stride, dilation=dil, residual=res, separable=k > 1)
    names = ("weight", "bias", "running_mean", "running_var")
    if k > 1:
        sd = {"mconv.0.conv.weight": op["dw_w"], "mconv.1.conv.weight": op["pw_w"][:, :, None]}
        sd.update({"mconv.2.layer.0." + n: v for n, v in zip(names, op["bn"])})
    else:
        sd = {"mconv.0.conv.weight": op["pw_w"][:, :, None]}
        sd.update({"mconv.1.layer.0." + n: v for n, v in zip(names, op["bn"])})
    if res:
        sd["res.0.conv.weight"] = op["res_w"][:, :, None]
        sd.update({"res.1.layer.0." + n: v for n, v in zip(names, op["res_bn"])})
    got, got_len = otcs.block_forward(spec, sd, "", op["x"], op["lens_t"], emulate_bf16=False)
    assert torch.equal(got_len.long(), len_out) and got.shape == ref.shape
    # the absolute sum of what the oracle adds up
    xm = op["x"].double().abs() * _mask(op["lens_t"], t)
    if k > 1:
        amid = F.conv1d(xm, op["dw_w"].double().abs(), None, stride, _pad(k, dil), dil, cin) * _mask(len_out, ref.shape[-1])
    else:
        amid = xm[:, :, ::stride]
    total = torch.einsum("oc,bct->bot", op["wf"].double().abs(), amid)
    terms = k + cin + 8
    sc, _ = _fold(op["bn"])
    total = total + (op["bn"][1].abs() + (op["bn"][2] * sc).abs()).double()[None, :, None]
    if res:
        rs, _ = _fold(op["res_bn"])
        total = total + torch.einsum("oc,bct->bot", op["rwf"].double().abs(), xm[:, :, ::stride][:, :, :ref.shape[-1]])
        total = total + (op["res_bn"][1].abs() + (op["res_bn"][2] * rs).abs()).double()[None, :, None]
        terms += cin
    _report("pin", f"restatement vs fp32 oracle {cin}->{cout} k={k} s={stride} d={dil}", (got.double() - ref).abs(), terms * 2.0 ** -23 * total)
    assert float(ref.abs().max()) > 0.1


def _source_instantiations():
    """The tuples the three files instantiate, read from their dispatch macros."""
    def body(name):
        text = open(os.path.join(CSRC, name)).read()
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
        return re.sub(r"^\s*#\s*define.*?(?<!\\)$", " ", text, flags=re.M | re.S)
    val = lambda s: {"true": 1, "false": 0}.get(s.strip(), None) if s.strip() in ("true", "false") else int(s)
    args = lambda m: [val(a) for a in m.split(",")]
    gen, split, logits = [], [], []
    k = body("tcs_kernel.hip")
    for m in re.findall(r"\bTS_TZ\(([^()]*)\)", k):
        tt, nt, s, tl, xj, np_ = args(m)
        gen.append(G(tt, nt, s, 1, 0, tl, 1, xj, np_))
    for m in re.findall(r"\bTS_ANY\(([^()]*)\)", k):
        tt, nt, s, dw, f32, tl = args(m)
        gen.append(G(tt, nt, s, dw, f32, tl, 0, 0, 0))
    for m in re.findall(r"\bTS_GEN\(([^()]*)\)", k):
        gen.append(G(*args(m)))
    sp = body("tcs_split.hip")
    for m in re.findall(r"\bTS_PIPE\(([^()]*)\)", sp):
        split.append(S(*args(m), 0))
    for m in re.findall(r"return\s+launch_split<([^<>]*)>\s*\(", sp):
        split.append(S(*args(m)))
    logits = re.findall(r"^int\s+launch_pw_logits\s*\(", body("pw_logits.hip"), flags=re.M)
    return gen, split, [LOGITS] * len(logits)


def test_every_instantiation_in_the_sources_has_a_checked_row():
    """An instantiation added to one of the three files without a row here (or a row whose kernel is gone) fails the CPU suite."""
    gen, split, logits = _source_instantiations()
    assert (len(gen), len(split), len(logits)) == (26, 12, 1), (len(gen), len(split), len(logits))
    assert len(set(gen)) == 26 and len(set(split)) == 12
    rows = {c["expect"] for c in CASES}
    assert not (rows & UNREACHABLE)
    assert rows | UNREACHABLE == set(gen) | set(split) | set(logits), (sorted(set(gen) | set(split) | set(logits) - rows - UNREACHABLE),
                                                                       sorted(rows - set(gen) - set(split) - set(logits)))
    assert len({c["name"] for c in CASES}) == len(CASES)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: one launch per row
# ---------------------------------------------------------------------------------------------------------------------
_KEPT = []


def _keep(x):
    """a device tensor that lives to the end of the test: a temporary is freed as soon as data_ptr() has returned, before the launch"""
    _KEPT.append(x)
    return x


@pytest.fixture(autouse=True)
def _release_kept():
    yield
    _KEPT.clear()


def _r8(n):
    return (n + 7) // 8 * 8


def _tail_zero_rows(x, lens, pitch):
    """x f32 [B][C][t] -> bf16 [B][C][pitch] inside a flat buffer with TS_GUARD_BYTES of zeros on both sides; 0 from each clip's length on"""
    from thunder_speech_amd import _lib
    b, c, t = x.shape
    guard = _lib.GUARD_BYTES // 2
    flat = _keep(torch.zeros(b * c * pitch + 2 * guard, dtype=BF, device="cuda"))
    rows = flat[guard: guard + b * c * pitch].view(b, c, pitch)
    rows[:, :, :t] = (x * _mask(lens, t).float()).to(BF).cuda()
    return rows


def _masked_rows(x, pitch):
    """x f32 [B][C][t] -> bf16 [B][C][pitch]: every frame of x (the kernel masks at the length), NaN from t to the pitch"""
    b, c, t = x.shape
    rows = _keep(torch.full((b, c, pitch), NAN, dtype=BF, device="cuda"))
    rows[:, :, :t] = x.to(BF).cuda()
    return rows


def _guarded_out(rows, pitch, dtype):
    """NaN rows with GUARD_ROWS rows of 7.0 before and after them"""
    buf = _keep(torch.full((rows + 2 * GUARD_ROWS, pitch), NAN, dtype=dtype, device="cuda"))
    buf[:GUARD_ROWS] = GUARD
    buf[GUARD_ROWS + rows:] = GUARD
    return buf


def _guards_ok(buf, rows, what):
    g = torch.cat([buf[:GUARD_ROWS], buf[GUARD_ROWS + rows:]])
    assert bool((g == GUARD).all()), f"{what}: a guard row next to the output was written"


def _record(L, _lib):
    rec = _lib.TcsLaunch()
    assert L.ts_tcs_last_launch(C.byref(rec)) == 0
    if rec.family == _lib.TCS_LAUNCH_GENERIC:
        tup = G(rec.tt, rec.nt, rec.stride, rec.dw, rec.out_f32, rec.tlds, rec.tz, rec.xj, rec.npass)
    elif rec.family == _lib.TCS_LAUNCH_SPLIT:
        tup = S(rec.npass, rec.xj, rec.wm, rec.dil, rec.se)
    elif rec.family == _lib.TCS_LAUNCH_LOGITS:
        tup = LOGITS
    else:
        tup = ("none",)
    return rec, tup


def _make_layer(op):
    from thunder_speech_amd import plan
    kw = dict(dw_w=op["dw_w"], pw_w=op["pw_w"], bn=op["bn"], kernel=op["k"], stride=op["stride"], dilation=op["dil"],
              padding=_pad(op["k"], op["dil"]), relu=op["relu"], out_fp32=op["f32"])
    if op["cres"]:
        kw.update(res_w=op["res_w"], res_bn=op["res_bn"], res_stride=op["res_stride"])
    layer = plan.make_tcs_layer("cuda", **kw)
    # the folded operands of the restatement are the device's: same values, bit for bit
    assert torch.equal(layer.bias[: op["cout"]].cpu(), op["shift"])
    return layer


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_instantiation_matches_the_float64_restatement(case):
    from thunder_speech_amd import _lib
    L = _lib.lib()
    op = _operands(case, seed=1 + CASES.index(case))
    layer = _make_layer(op)
    b, cin, cout, t = len(case["lens"]), case["cin"], case["cout"], case["t"]
    tz = case["mode"] == "tz"
    t_out = layer.out_size(t)
    pitch_in, pitch_out = _lib.time_pitch(t), _lib.time_pitch(t_out)
    if case["refuse"] == "taps_raw":
        assert layer.taps_raw is not None
        layer.taps_raw = None
    elif case["refuse"] == "pitch":
        pitch_out = _r8(t_out)                                     # holds the generic kernel's stores (they stop at the pitch), not the split kernel's tiles
    lens = op["lens_t"]
    rows = _tail_zero_rows if tz else (lambda x, ln, p: _masked_rows(x, p))
    xd = rows(op["x"], lens, pitch_in)
    xr = rows(op["xres"], lens, pitch_in) if case["cres"] else None
    ld = _keep(lens.to(torch.int32).cuda())
    dtype = torch.float32 if case["f32"] else BF
    out = _guarded_out(b * cout, pitch_out, dtype)
    y = out[GUARD_ROWS: GUARD_ROWS + b * cout]
    d = layer.desc(b, t, pitch_in, pitch_out, tz, case["zero_tail"], pitch_res=pitch_in, t_res=t)
    d.t_out = t_out
    n_dw = 4 * layer.nk
    if case["phase"]:
        d.flags |= _lib.TCS_TAPS_PHASE
        d.dw_taps, d.dw_ksteps, d.dw_taps_raw = layer.taps_phase.data_ptr(), layer.nk_phase, layer.taps_phase_raw.data_ptr()
        n_dw = 4 * layer.nk_phase
    if case["se"]:
        se_y = _tail_zero_rows(op["se_y"], lens, pitch_out)
        gate = _keep(op["gate"].cuda())
        d.se_y, d.se_gate = se_y.data_ptr(), gate.data_ptr()
    stats = None
    if case["stats"]:
        tf = L.ts_tcs_pointwise_tile_frames(b, cout, t_out)
        n_st = (t_out + tf - 1) // tf
        stats = _keep(torch.full((cout + 1, b * n_st * 2), NAN, dtype=torch.float32, device="cuda"))
        stats[cout] = GUARD
        d.stats = stats.data_ptr()
    what = case["name"]
    st = L.ts_tcs_subblock_fwd(C.byref(d), xd.data_ptr(), ld.data_ptr(), xr.data_ptr() if xr is not None else None,
                               ld.data_ptr() if xr is not None else None, y.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert st == 0, f"{what}: ts_tcs_subblock_fwd returned {st}"
    rec, tup = _record(L, _lib)
    torch.cuda.synchronize()
    assert tup == case["expect"], f"{what}: launched {tup}, the row names {case['expect']}"
    assert rec.grid >= 1 and rec.n_tiles == b * rec.n_tt * rec.n_z and rec.grid <= rec.n_tiles and rec.lds_bytes > 0
    if tup[0] == "generic":
        assert rec.n_tt == (t_out + rec.tt - 1) // rec.tt and rec.n_z == ((cout + 31) // 32 * 32 + 128 * rec.nt - 1) // (128 * rec.nt)
    if tup[0] == "split":
        assert rec.n_tt == (t_out + 96 * rec.wm - 1) // (96 * rec.wm) and rec.n_z == ((cout + 31) // 32 * 32 + 512 // rec.wm - 1) // (512 // rec.wm)
        assert rec.xcd == (1 if rec.grid % 8 == 0 else 0)
    if case["xcd"] is not None:
        assert rec.xcd == case["xcd"], (what, rec.xcd, rec.grid)
    if case["wrap"]:
        assert rec.n_tiles > rec.grid, f"{what}: {rec.n_tiles} tiles on {rec.grid} workgroups: the persistent loop does not wrap"
    if case["tile_frames"] is not None:
        assert L.ts_tcs_pointwise_tile_frames(b, cout, t_out) == case["tile_frames"] == rec.tt
    if case["tt_logits"] is not None:
        assert rec.tt == case["tt_logits"]

    ref, bound, len_out = _reference(op, n_dw)
    assert ref.shape == (b, cout, t_out)
    got = y.view(b, cout, pitch_out)[:, :, :t_out].double().cpu()
    kind = ("f32" if case["f32"] else "se" if case["se"] else "bf16") + "|" + tup[0]
    _report(kind, what, (got - ref).abs(), bound)
    _guards_ok(out, b * cout, what)
    if case["zero_tail"]:
        for i, n in enumerate(len_out.tolist()):
            assert bool((got[i, :, n:] == 0).all()), f"{what}: clip {i} is not exactly 0 from frame {n} on"
    else:
        assert any(n < t_out for n in len_out.tolist()) and float(ref.abs().max()) > 0
    assert float(ref.abs().max()) > 0.1
    if stats is not None:
        assert bool((stats[cout] == GUARD).all()), f"{what}: the guard row behind the statistics was written"
        tf = case["tile_frames"]
        n_st = (t_out + tf - 1) // tf
        s = F.pad(got, (0, n_st * tf - t_out)).view(b, cout, n_st, tf)
        s1, a1, s2 = s.sum(-1), s.abs().sum(-1), (s * s).sum(-1)
        gs = stats[:cout].double().cpu().view(cout, b, n_st, 2).permute(1, 0, 2, 3)
        rho = U16 / (1 - U16)
        _report("stats-sum|generic", what, (gs[..., 0] - s1).abs(), (rho + (tf + 1) * U32 * (1 + rho)) * a1)
        _report("stats-sumsq|generic", what, (gs[..., 1] - s2).abs(), (rho * (2 + rho) + (tf + 1) * U32 * (1 + rho) ** 2) * s2)


@pytest.mark.gpu
def test_the_record_is_cleared_by_a_refused_call_and_is_per_call():
    """A launch leaves its record; the next call on the thread that is refused before any launcher leaves "nothing launched"."""
    from thunder_speech_amd import _lib
    L = _lib.lib()
    case = next(c for c in CASES if c["name"] == "split-np2-wm2")
    op = _operands(case, seed=99)
    layer = _make_layer(op)
    b, t = len(case["lens"]), case["t"]
    pitch = _lib.time_pitch(t)
    xd = _tail_zero_rows(op["x"], op["lens_t"], pitch)
    ld = _keep(op["lens_t"].to(torch.int32).cuda())
    out = _guarded_out(b * case["cout"], pitch, BF)
    y = out[GUARD_ROWS: GUARD_ROWS + b * case["cout"]]
    d = layer.desc(b, t, pitch, pitch, True, True)
    args = (xd.data_ptr(), ld.data_ptr(), None, None, y.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert L.ts_tcs_subblock_fwd(C.byref(d), *args) == 0
    rec, tup = _record(L, _lib)
    assert tup == case["expect"] and rec.grid > 0
    d.stride = 3
    assert L.ts_tcs_subblock_fwd(C.byref(d), *args) == _lib.TS_EUNSUPPORTED
    rec, tup = _record(L, _lib)
    assert tup == ("none",) and bytes(rec) == bytes(_lib.TcsLaunch())
    torch.cuda.synchronize()


def test_the_unreachable_instantiation_is_refused_by_the_dispatcher():
    """UNREACHABLE above: stride 2, at most 256 output channels, more than 24 k-steps -- the staged row exceeds 320 frames for every such layer, and
    ts_tcs_subblock_fwd answers TS_EUNSUPPORTED before any launcher (made-up addresses, never dereferenced)."""
    from thunder_speech_amd import _lib, plan
    L = _lib.lib()
    A = 0x10000
    for k in (95, 101, 151):
        nk = plan.dw_ksteps(k, 2, 1, _pad(k, 1))
        assert nk > 24
        for flags in (0, _lib.TCS_IN_TAILZERO | _lib.TCS_OUT_ZERO_TAIL):
            d = _lib.TcsDesc(batch=2, c_in=64, c_out=256, t_in=300, t_out=150, pitch_in=768, pitch_out=640, kernel=k, stride=2, dilation=1,
                             padding=_pad(k, 1), depthwise=1, dw_taps=A, dw_ksteps=nk, pw_w=A, bias=A, flags=flags)
            assert L.ts_tcs_subblock_fwd(C.byref(d), A, A, None, None, A, None) == _lib.TS_EUNSUPPORTED
            rec = _lib.TcsLaunch()
            assert L.ts_tcs_last_launch(C.byref(rec)) == 0 and rec.family == _lib.TCS_LAUNCH_NONE
    # the smallest k-step count that reads its taps from global memory already needs 248 + 4 x 27 = 356 frames
    assert 3 * 32 * 2 + 4 * (7 * 2 + 27) > 64 * 5
