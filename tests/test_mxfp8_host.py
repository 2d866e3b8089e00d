"""precision="mxfp8" on the CPU: the staged header include_staged/thunder_speech_amd/mxfp8.h through `_lib.STAGED` and the built library's symbols,
include/ and `_lib.COMPANIONS` untouched by it, the mode's refusals (a check that needs no GPU), and the restated quantiser of
tests/mxfp8_restatement.py on hand-made blocks -- the same blocks tests/test_gpu_mxfp8_kernels.py feeds to ts_mx_quantize_rows."""
import ctypes
import glob
import os
import subprocess
import types

import pytest
import torch

from mxfp8_restatement import E4M3_MAX, fake_quant, handmade_blocks, mx_dequantize, mx_exponent, mx_quantize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, i32, i64, f32, cint = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_int

NAMES = ["ts_mxfp8_abi_version", "ts_mx_quantize_rows", "ts_mx_layernorm_fwd", "ts_mx_pack_w_scale_bytes", "ts_mx_pack_w", "ts_mx_gemm_nt"]
SIGNATURES = {
    "ts_mxfp8_abi_version": (cint, []),
    "ts_mx_quantize_rows": (cint, [vp, i32, i64, i64, i32, vp, i64, vp, i64, vp]),
    "ts_mx_layernorm_fwd": (cint, [vp, vp, vp, vp, vp, f32, i64, i32, vp, vp, i64, vp, i64, vp]),
    "ts_mx_pack_w_scale_bytes": (i64, [i32, i32]),
    "ts_mx_pack_w": (cint, [vp, i64, vp, i64, i32, i32, vp, vp, vp]),
    "ts_mx_gemm_nt": (cint, [vp, i64, vp, i64, vp, vp, vp, i32, vp, i64, vp, i64, vp, i64, vp, i64, i64, i32, i32, vp]),
}


def test_staged_header_parses_and_declares_exactly_its_names():
    from thunder_speech_amd import _lib
    assert list(_lib.STAGED) == ["mxfp8"]
    h = _lib.STAGED["mxfp8"]
    assert h.path == os.path.join(ROOT, "include_staged", "thunder_speech_amd", "mxfp8.h")
    assert list(h.signatures) == NAMES and h.signatures == SIGNATURES
    assert (h.version_define, h.version_function, h.abi_version) == ("TS_MXFP8_ABI_VERSION", "ts_mxfp8_abi_version", 1)
    assert h.structs == {}
    assert h.defines == {"TS_MXFP8_ABI_VERSION": 1, "TS_MX_GEMM_TILE_ROWS": 128, "TS_MX_GEMM_TILE_COLS": 128, "TS_MX_EP_BF16": 0, "TS_MX_EP_ACCUM": 1,
                         "TS_MX_EP_GELU_MX": 2}
    # no name of it is declared by the core header or a companion
    others = set(_lib.SIGNATURES).union(*(c.signatures for c in _lib.COMPANIONS.values()))
    assert not others & set(NAMES)


def test_built_library_defines_every_staged_name():
    from thunder_speech_amd import build as b
    path = b.build(verbose=False)
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert not [n for n in NAMES if n not in defined]


def test_include_directory_and_companions_are_unchanged():
    from thunder_speech_amd import _lib
    assert len(_lib.COMPANIONS) == 14 and "mxfp8" not in _lib.COMPANIONS
    assert len(glob.glob(os.path.join(ROOT, "include", "thunder_speech_amd", "*.h"))) == 14
    assert sorted(os.listdir(os.path.join(ROOT, "include"))) == ["thunder_speech_amd", "thunder_speech_amd.h"]
    assert len(_lib.SIGNATURES) == len(_lib.EXPORTED_SYMBOLS) == 123 and _lib.ABI_VERSION == 15


def test_editing_the_staged_header_makes_the_library_stale(tmp_path, monkeypatch):
    from thunder_speech_amd import _lib, build as b
    header = _lib.STAGED["mxfp8"].path
    assert header in b.header_deps()
    lib = tmp_path / "lib.so"
    lib.write_bytes(b"")
    monkeypatch.setattr(b, "lib_path", lambda: str(lib))
    real = glob.glob
    monkeypatch.setattr(b, "sources", lambda: [])
    monkeypatch.setattr(b.glob, "glob", lambda pat, **kw: [p for p in real(pat, **kw) if p == header])
    mtime = os.path.getmtime(header)
    os.utime(lib, (mtime + 10, mtime + 10))
    assert not b.needs_build()
    os.utime(lib, (mtime - 10, mtime - 10))
    assert b.needs_build()


# ---- the mode's refusals ---------------------------------------------------------------------------------------------
def _cfg(**kw):
    base = dict(model_type="wav2vec2", hidden_size=768, intermediate_size=3072, num_attention_heads=12, do_stable_layer_norm=False,
                adapter_attn_dim=None)
    base.update(kw)
    return types.SimpleNamespace(**base)


@pytest.mark.parametrize("model_type", ["wav2vec2", "hubert", "unispeech", "unispeech-sat", "data2vec-audio"])
def test_refusal_check_accepts_the_families_in_scope(model_type):
    from thunder_speech_amd.huggingface.encoder import check_mxfp8_config
    check_mxfp8_config(_cfg(model_type=model_type))
    check_mxfp8_config(_cfg(model_type=model_type, do_stable_layer_norm=True, hidden_size=1024, intermediate_size=4096, num_attention_heads=16))
    check_mxfp8_config(_cfg(model_type=model_type, hidden_size=1280, intermediate_size=5120, num_attention_heads=16))       # head_dim 80


@pytest.mark.parametrize("kw,words", [
    (dict(model_type="wavlm"), ("wavlm", "gate")),
    (dict(model_type="wav2vec2-conformer"), ("wav2vec2-conformer",)),
    (dict(model_type="sew"), ("sew",)),
    (dict(do_stable_layer_norm=True, adapter_attn_dim=16), ("adapter_attn_dim",)),
    (dict(hidden_size=192, num_attention_heads=3, intermediate_size=768), ("hidden_size=192", "128")),
    (dict(intermediate_size=3000), ("intermediate_size=3000", "128")),
])
def test_refusal_check_names_each_refused_configuration(kw, words):
    from thunder_speech_amd.huggingface.encoder import check_mxfp8_config
    with pytest.raises(NotImplementedError) as e:
        check_mxfp8_config(_cfg(**kw))
    assert "mxfp8" in str(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_assigning_the_adapters_precision_retires_captured_graphs():
    """`encoder.precision = ...` moves `_param_epoch`, which BaseCTCModule._weights_stamp folds into the stamp its inference graphs are keyed on; the
    same value again moves nothing."""
    from torch import nn
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt

    class Stub(nn.Module):
        config = _cfg()
    enc = HuggingFaceEncoderAdapt(Stub(), precision="bf16")
    e0 = enc._param_epoch
    enc.precision = "bf16"
    assert enc._param_epoch == e0 and enc.precision == "bf16"
    enc.precision = "mxfp8"
    assert enc._param_epoch == e0 + 1 and enc.precision == "mxfp8"
    enc.precision = "bf16"
    assert enc._param_epoch == e0 + 2
    # an adapter restored from a pickle written while `precision` was a plain attribute: the value sits in __dict__ under that name
    old = HuggingFaceEncoderAdapt(Stub(), precision="bf16")
    del old.__dict__["_precision"]
    old.__dict__["precision"] = "fp32"
    assert old.precision == "fp32"
    old.precision = "bf16"
    assert old.precision == "bf16"
    with pytest.raises(NotImplementedError, match="wavlm"):
        class Wavlm(nn.Module):
            config = _cfg(model_type="wavlm")
        HuggingFaceEncoderAdapt(Wavlm(), precision="mxfp8")


def test_unknown_precision_is_still_a_value_error():
    from thunder_speech_amd.huggingface.encoder import Wav2Vec2Plan
    with pytest.raises(ValueError, match="int3"):
        Wav2Vec2Plan(_cfg(conv_kernel=[10], conv_stride=[5], conv_dim=[32]), {}, "cpu", precision="int3")


# ---- the restated quantiser ----------------------------------------------------------------------------------------------
def _check_blocks(v):
    q, s = mx_quantize(v)
    v = v.to(torch.float32)
    assert q.dtype == torch.uint8 and s.dtype == torch.uint8 and q.shape == v.shape and s.shape == (v.shape[0], v.shape[1] // 32)
    assert not bool(((q & 0x7F) == 0x7F).any()), "an element is NaN (e4m3fn: S.1111.111)"
    blocks = v.double().reshape(v.shape[0], -1, 32)
    amax = blocks.abs().amax(-1)
    e = s.double() - 127.0
    deq = mx_dequantize(q, s).reshape(blocks.shape)
    err = (deq - blocks).abs()
    two_e = torch.pow(torch.tensor(2.0, dtype=torch.float64), e).unsqueeze(-1)
    normal = blocks.abs() >= 2.0 ** -6 * two_e                                    # lands in e4m3's normal range
    assert bool((err[normal] <= 2.0 ** -4 * blocks.abs()[normal]).all())
    assert bool((err <= torch.where(normal, 2.0 ** -4 * blocks.abs(), 2.0 ** -10 * two_e)).all())
    # the smallest exponent at which nothing saturates (or the clamp); zero blocks: byte 0 and zero bytes
    nz = amax > 0
    assert bool((amax[nz] / two_e.squeeze(-1)[nz] <= E4M3_MAX).all())
    assert bool(((amax[nz] / two_e.squeeze(-1)[nz] * 2.0 > E4M3_MAX) | (e[nz] == -127)).all())
    assert bool((s[~nz] == 0).all()) and bool((q.reshape(blocks.shape)[~nz] == 0).all())
    # signs survive
    signed = (deq != 0)
    assert bool((torch.sign(deq[signed]) == torch.sign(blocks[signed])).all())
    return q, s


def test_restated_quantiser_on_handmade_blocks():
    hb = handmade_blocks()
    q, s = _check_blocks(hb)
    named = {}
    for row, (base, p) in enumerate((b, p) for b in (448.0, 449.0, 256.0, 255.9) for p in (0, -3, 5, -20)):
        named[(base, p)] = int(s[row, 0]) - 127
    for p in (0, -3, 5, -20):
        assert named[(448.0, p)] == p            # 448 2^p fits exactly at e = p
        assert named[(449.0, p)] == p + 1        # 449 would saturate at e = p: the plain OCP rule clips it
        assert named[(256.0, p)] == p
        assert named[(255.9, p)] == p            # floor(log2) - 8 = p - 1 would put it at 511.8: one up
    n = 16
    assert int(s[n, 0]) == 0 and int(s[n + 1, 0]) == 0 and not bool(q[n:n + 2].any())          # zero blocks (one with a -0.0)
    assert int(q[n + 2, 17]) != 0                                                               # the single tiny value is not lost
    assert int(s[n + 3, 0]) == 0 and int(q[n + 3, 0]) == 0x48                                   # lower clamp: 2^-125 2^127 = 4.0
    assert int(s[n + 4, 0]) == 127 + 120                                                        # the largest f32: e = 120, below the upper clamp
    sub = q[n + 5]
    assert [int(x) for x in sub[1:8]] == [2, 2, 4, 0, 0, 8, 0x84]                              # ties to even among the subnormals; 7.6 -> 8 = the first normal
    assert bool((q[n + 6] & 0x80)[hb[n + 6] != 0].all())                                        # the negative block keeps its signs


def test_restated_quantiser_on_random_rows_and_bf16_sources():
    g = torch.Generator().manual_seed(5)
    v = torch.randn(9, 384, generator=g) * torch.logspace(-6, 6, 9).unsqueeze(-1)
    _check_blocks(v)
    _check_blocks(v.to(torch.bfloat16))
    # a single product of Gaussian operands: about 4 % relative rms error (the issue's figure), far below 10 %
    a, b = torch.randn(64, 1024, generator=g), torch.randn(48, 1024, generator=g)
    ref = a.double() @ b.double().t()
    got = fake_quant(a).double() @ fake_quant(b).double().t()
    rel = float((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
    assert 0.02 < rel < 0.06, rel


def test_exponent_comes_from_the_bits():
    amax = torch.tensor([448.0, 448.0 * (1 + 2.0 ** -23), 447.99997, 1.75, 1.7500001, 2.0 ** -126, 2.0 ** -140, 0.0])
    assert mx_exponent(amax).tolist() == [0, 1, 0, -8, -7, -127, -127, -127]
