"""Adapter-only fine-tuning of MMS checkpoints on the CPU: the sixth companion header (include/thunder_speech_amd_mms_adapter_train.h) next to the
unchanged other headers, its binding in _lib, the symbols of the built library, and the regime -- which models train mode refuses by name and
what HuggingFaceEncoderAdapt.adapter_finetuning() sets up."""
import ctypes
import glob
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "thunder_speech_amd_mms_adapter_train.h")
NAMES = sorted(["ts_mms_adapter_train_abi_version", "ts_mms_attn_adapter_train_fwd", "ts_mms_attn_adapter_train_bwd_workspace",
                "ts_mms_attn_adapter_train_bwd"])
# tests/test_mms_host.py's model: hidden 160, 2 heads (head_dim 80), adapter 16
CFG = dict(hidden_size=160, num_hidden_layers=2, num_attention_heads=2, intermediate_size=320, feat_extract_norm="layer", conv_bias=True,
           do_stable_layer_norm=True, vocab_size=32, conv_dim=(32,) * 7, conv_kernel=(10, 3, 3, 3, 3, 2, 2),
           conv_stride=(5, 2, 2, 2, 2, 2, 2), num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, pad_token_id=0, adapter_attn_dim=16)


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ts_[a-z0-9_]+)\s*\(", src)))


# ---- header and ABI ----------------------------------------------------------------------------------------------------------------------------
def test_companion_header_parses_and_declares_exactly_the_four_names():
    from thunder_speech_amd import _lib
    assert _lib.MMS_ADAPTER_TRAIN_HEADER == HEADER
    sigs, structs, defines = _lib.read_header(open(HEADER).read())
    assert defines["TS_MMS_ADAPTER_TRAIN_ABI_VERSION"] == 1 and _lib.MMS_ADAPTER_TRAIN_ABI_VERSION == 1 and not structs
    assert sorted(sigs) == _declared(HEADER) == NAMES
    assert _lib.MMS_ADAPTER_TRAIN_SIGNATURES == sigs
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert sigs["ts_mms_adapter_train_abi_version"] == (ctypes.c_int, [])
    assert sigs["ts_mms_attn_adapter_train_fwd"] == (ctypes.c_int, [vp, i64, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp])
    assert sigs["ts_mms_attn_adapter_train_bwd_workspace"] == (i64, [i64, i32, i32])
    assert sigs["ts_mms_attn_adapter_train_bwd"] == (ctypes.c_int, [vp, vp, i64, i32, i32] + [vp] * 13 + [i32, vp])


def test_no_name_is_declared_twice_and_the_older_headers_are_at_their_versions():
    from thunder_speech_amd import _lib
    headers = sorted(glob.glob(os.path.join(ROOT, "include", "*.h")))
    assert len(headers) == 7
    names = [n for h in headers for n in _declared(h)]
    assert len(names) == len(set(names))
    assert len(_declared(os.path.join(ROOT, "include", "thunder_speech_amd.h"))) == 123 and _lib.ABI_VERSION == 15
    assert (_lib.WAVLM_ABI_VERSION, _lib.WAVLM_TRAIN_ABI_VERSION, _lib.CONFORMER_ABI_VERSION, _lib.MMS_ABI_VERSION,
            _lib.MMS_TRAIN_ABI_VERSION) == (1, 1, 1, 1, 1)
    for table in (_lib.SIGNATURES, _lib.WAVLM_SIGNATURES, _lib.WAVLM_TRAIN_SIGNATURES, _lib.CONFORMER_SIGNATURES, _lib.MMS_SIGNATURES,
                  _lib.MMS_TRAIN_SIGNATURES):
        assert not set(table) & set(NAMES)


def test_built_library_defines_the_four_symbols():
    from thunder_speech_amd import build as b
    path = b.build(verbose=False)
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert set(NAMES) <= defined


# ---- the regime --------------------------------------------------------------------------------------------------------------------------------
def _adapt(train_precision="fp32", **kw):
    transformers = pytest.importorskip("transformers")
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    model = transformers.Wav2Vec2Model(transformers.Wav2Vec2Config(**{**CFG, **kw}))
    return model, HuggingFaceEncoderAdapt(model, train_precision=train_precision)


def _train_forward_error(enc):
    enc.train()
    with pytest.raises(Exception) as e:
        enc(torch.zeros(1, 4000), torch.tensor([4000]))             # CPU tensors: a refusal by name comes first, else the GPU check (no CPU path)
    return e.value


@pytest.mark.parametrize("train_precision", ["fp32", "bf16"])
def test_train_mode_is_refused_by_name_until_the_base_is_frozen(train_precision):
    model, enc = _adapt(train_precision)
    err = _train_forward_error(enc)
    assert isinstance(err, NotImplementedError) and "adapter_attn_dim=16" in str(err) and "adapter_finetuning" in str(err)
    enc.adapter_finetuning()
    err = _train_forward_error(enc)
    assert isinstance(err, RuntimeError) and not isinstance(err, NotImplementedError), err          # the GPU check is reached
    # one base parameter made trainable again: the refusal is back, and names it
    model.encoder.layers[1].attention.q_proj.weight.requires_grad_(True)
    err = _train_forward_error(enc)
    assert isinstance(err, NotImplementedError) and "adapter_attn_dim=16" in str(err) and "q_proj.weight" in str(err)


def test_adapter_finetuning_returns_transformers_adapters_and_freezes_everything_else():
    model, enc = _adapt()
    named = enc.adapter_finetuning()
    want = {"original_encoder." + k for k in model._get_adapters()}
    assert set(named) == want and len(want) == 12
    sd = enc.state_dict()
    assert all(k in sd for k in named)
    assert {n for n, p in enc.named_parameters() if p.requires_grad} == want
    assert all(named[n] is p for n, p in enc.named_parameters() if n in named)


def test_a_model_without_adapters_has_nothing_to_fine_tune():
    _, enc = _adapt(adapter_attn_dim=None, num_attention_heads=4)
    with pytest.raises(ValueError, match="adapter"):
        enc.adapter_finetuning()


def test_init_gives_fresh_adapters_and_leaves_the_base():
    model, enc = _adapt()
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    enc.adapter_finetuning(init=False)
    assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items())
    enc.adapter_finetuning(init=True)
    after = model.state_dict()
    assert not torch.equal(after["encoder.layers.0.adapter_layer.linear_2.weight"], before["encoder.layers.0.adapter_layer.linear_2.weight"])
    assert not torch.equal(after["encoder.layers.1.adapter_layer.linear_1.weight"], before["encoder.layers.1.adapter_layer.linear_1.weight"])
    assert all(torch.equal(v, before[k]) for k, v in after.items() if "adapter_layer" not in k)
