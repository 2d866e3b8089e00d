"""Fine-tuning of HuBERT, UniSpeech, UniSpeech-SAT and data2vec-audio checkpoints on the CPU: train mode gets past the refusal by name to the GPU
check for every one of them, what data2vec-audio still refuses (by name, with the wording the other families get), and the seventh companion header
(include/thunder_speech_amd/posconv_stack_train.h, the first in its directory) next to the unchanged seven headers of include/."""
import ctypes
import glob
import os
import re
import subprocess

import pytest
import torch

transformers = pytest.importorskip("transformers")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "thunder_speech_amd", "posconv_stack_train.h")
NAMES = sorted(["ts_posconv_stack_train_abi_version", "ts_posconv_stack_conv_workspace", "ts_posconv_stack_conv", "ts_posconv_stack_norm_gelu_fwd",
                "ts_posconv_stack_norm_gelu_bwd_workspace", "ts_posconv_stack_norm_gelu_bwd"])
TINY = dict(vocab_size=32, hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128, conv_dim=(32, 32, 32), conv_stride=(5, 2, 2),
            conv_kernel=(10, 3, 2), num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4)
FAMILIES = {
    "hubert": lambda **kw: transformers.HubertModel(transformers.HubertConfig(**{**TINY, "feat_proj_layer_norm": False, **kw})),
    "hubert_large": lambda **kw: transformers.HubertModel(transformers.HubertConfig(**{**TINY, "feat_proj_layer_norm": True, "do_stable_layer_norm": True,
                                                                                       "feat_extract_norm": "layer", "conv_bias": True, **kw})),
    "unispeech": lambda **kw: transformers.UniSpeechModel(transformers.UniSpeechConfig(**{**TINY, **kw})),
    "unispeech-sat": lambda **kw: transformers.UniSpeechSatModel(transformers.UniSpeechSatConfig(**{**TINY, **kw})),
    "data2vec-audio": lambda **kw: transformers.Data2VecAudioModel(transformers.Data2VecAudioConfig(**{**TINY, "num_conv_pos_embeddings": 3,
                                                                                                       "conv_pos_kernel_size": 19, **kw})),
}


def _adapt(family, train_precision="fp32", **kw):
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    model = FAMILIES[family](**kw)
    model.feature_extractor._freeze_parameters()               # HubertModel and UniSpeechSatModel have no freeze_feature_encoder for the adapter to call
    return HuggingFaceEncoderAdapt(model, train_precision=train_precision)


# ---- the regime --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("train_precision", ["fp32", "bf16"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_train_mode_gets_past_the_refusal_by_name_to_the_gpu_check(family, train_precision):
    from thunder_speech_amd.huggingface import train as T
    enc = _adapt(family, train_precision).train()
    T.refuse_untrainable(enc, train_precision == "bf16")       # nothing to refuse
    with pytest.raises(RuntimeError) as e:
        enc(torch.zeros(1, 4000), torch.tensor([4000]))        # CPU tensors: what is left is the GPU check (there is no CPU path)
    assert not isinstance(e.value, NotImplementedError), e.value
    assert enc.original_encoder.config.model_type in T.TRAINABLE_MODEL_TYPES


def test_hubert_base_has_no_feature_projection_layer_norm_and_hubert_large_has_one():
    assert not hasattr(_adapt("hubert").original_encoder.feature_projection, "layer_norm")
    assert hasattr(_adapt("hubert_large").original_encoder.feature_projection, "layer_norm")


def test_data2vec_audio_still_refuses_what_the_other_families_refuse_with_the_same_wording():
    from thunder_speech_amd.huggingface import train as T
    for mixed in (False, True):
        with pytest.raises(NotImplementedError, match="mask_feature_prob > 0 is not supported"):
            T.refuse_untrainable(_adapt("data2vec-audio", mask_feature_prob=0.1), mixed)
        with pytest.raises(NotImplementedError, match=r"add_adapter=True is inference-only \(the adapter layers have no backward here\)"):
            T.refuse_untrainable(_adapt("data2vec-audio", add_adapter=True), mixed)
        enc = _adapt("data2vec-audio")
        next(enc.original_encoder.feature_extractor.parameters()).requires_grad_(True)
        with pytest.raises(NotImplementedError, match=r"the conv feature extractor is frozen \(freeze_feature_encoder\); 1 of its parameters"):
            T.refuse_untrainable(enc, mixed)


def test_the_conformer_is_still_refused_by_name_in_both_places():
    from thunder_speech_amd.huggingface import train as T
    assert "wav2vec2-conformer" not in T.TRAINABLE_MODEL_TYPES
    assert set(T.TRAINABLE_MODEL_TYPES) == {"wav2vec2", "wavlm", "hubert", "unispeech", "unispeech-sat", "data2vec-audio"}


# ---- header and ABI ----------------------------------------------------------------------------------------------------------------------------
def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ts_[a-z0-9_]+)\s*\(", src)))


def test_companion_header_parses_and_declares_exactly_the_six_names():
    from thunder_speech_amd import _lib
    assert _lib.POSCONV_STACK_TRAIN_HEADER == HEADER
    sigs, structs, defines = _lib.read_header(open(HEADER).read())
    assert defines["TS_POSCONV_STACK_TRAIN_ABI_VERSION"] == 1 and _lib.POSCONV_STACK_TRAIN_ABI_VERSION == 1 and not structs
    assert sorted(sigs) == _declared(HEADER) == NAMES
    assert _lib.POSCONV_STACK_TRAIN_SIGNATURES == sigs
    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    assert sigs["ts_posconv_stack_train_abi_version"] == (ctypes.c_int, [])
    assert sigs["ts_posconv_stack_conv_workspace"] == (i64, [i32, i32, i32, i32])
    assert sigs["ts_posconv_stack_conv"] == (ctypes.c_int, [vp, i32, i32, i32, vp, i32, i32, i32, vp, vp, vp])
    assert sigs["ts_posconv_stack_norm_gelu_fwd"] == (ctypes.c_int, [vp, vp, f32, i64, i32, vp, vp])
    assert sigs["ts_posconv_stack_norm_gelu_bwd_workspace"] == (i64, [i64, i32])
    assert sigs["ts_posconv_stack_norm_gelu_bwd"] == (ctypes.c_int, [vp, vp, vp, f32, i64, i32, vp, vp, vp, vp])


def test_no_other_header_or_table_holds_the_names_and_include_keeps_its_seven_files():
    from thunder_speech_amd import _lib
    assert len(glob.glob(os.path.join(ROOT, "include", "*.h"))) == 7
    every = sorted(glob.glob(os.path.join(ROOT, "include", "**", "*.h"), recursive=True))
    assert HEADER in every and len(every) == 8
    for h in every:
        if h != HEADER:
            assert not set(_declared(h)) & set(NAMES), h
    for table in (_lib.SIGNATURES, _lib.WAVLM_SIGNATURES, _lib.WAVLM_TRAIN_SIGNATURES, _lib.CONFORMER_SIGNATURES, _lib.MMS_SIGNATURES,
                  _lib.MMS_TRAIN_SIGNATURES, _lib.MMS_ADAPTER_TRAIN_SIGNATURES):
        assert not set(table) & set(NAMES)
    assert len(_declared(os.path.join(ROOT, "include", "thunder_speech_amd.h"))) == 123 and _lib.ABI_VERSION == 15


def test_built_library_defines_the_six_symbols():
    from thunder_speech_amd import build as b
    path = b.build(verbose=False)
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert set(NAMES) <= defined


def test_editing_the_header_makes_the_library_stale(tmp_path, monkeypatch):
    """build.needs_build() looks at include/thunder_speech_amd/*.h too: a header newer than the library asks for a rebuild."""
    from thunder_speech_amd import build as b
    lib = tmp_path / "lib.so"
    lib.write_bytes(b"")
    monkeypatch.setattr(b, "lib_path", lambda: str(lib))
    # only the headers of that directory count here: every other dependency is taken out of the comparison
    real = glob.glob
    monkeypatch.setattr(b, "sources", lambda: [])
    monkeypatch.setattr(b.glob, "glob", lambda pat, **kw: real(pat, **kw) if os.path.dirname(pat) == os.path.dirname(HEADER) else [])
    mtime = os.path.getmtime(HEADER)
    os.utime(lib, (mtime + 10, mtime + 10))
    assert not b.needs_build()
    os.utime(lib, (mtime - 10, mtime - 10))
    assert b.needs_build()
