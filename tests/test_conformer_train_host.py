"""wav2vec2-conformer fine-tuning on the CPU: the companion C header inside the package (thunder_speech_amd/abi/conformer_train.h) next to the
unchanged core ABI and the other companions, and the refusals of huggingface/conformer_train.py, each by name and before any device work (CPU
tensors: a refusal that came later would be the GPU check's RuntimeError instead)."""
import ctypes
import glob
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "thunder_speech_amd", "abi", "conformer_train.h")
NAMES = sorted(["ts_conformer_train_abi_version", "ts_conformer_glu_dwconv_train_fwd_workspace", "ts_conformer_glu_dwconv_train_fwd",
                "ts_conformer_bn_stats", "ts_conformer_bn_act_cast", "ts_conformer_bn_act_bwd_sums_workspace", "ts_conformer_bn_act_bwd_sums",
                "ts_conformer_glu_dwconv_train_bwd_workspace", "ts_conformer_glu_dwconv_train_bwd", "ts_conformer_rotary_bwd",
                "ts_conformer_ffn_act_cast", "ts_conformer_ffn_act_bwd"])


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ts_[a-z0-9_]+)\s*\(", src)))


def test_companion_header_parses_declares_exactly_the_table_and_reports_its_version():
    from thunder_speech_amd import _lib
    assert _lib.CONFORMER_TRAIN_HEADER == HEADER
    text = open(HEADER).read()
    sigs, structs, defines = _lib.read_header(text)
    assert defines["TS_CONFORMER_TRAIN_ABI_VERSION"] == 1 and _lib.CONFORMER_TRAIN_ABI_VERSION == 1 and not structs
    assert sorted(sigs) == _declared(HEADER) == NAMES == sorted(_lib.CONFORMER_TRAIN_SIGNATURES)
    assert _lib.CONFORMER_TRAIN_SIGNATURES == sigs
    assert not re.search(r"\b(size_t|double)\b", re.sub(r"/\*.*?\*/", "", text, flags=re.S))          # only the types read_header maps
    vp, i32, i64, u64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float
    assert sigs["ts_conformer_train_abi_version"] == (ctypes.c_int, [])
    assert sigs["ts_conformer_glu_dwconv_train_fwd_workspace"] == (i64, [i32, i32, i32])
    assert sigs["ts_conformer_glu_dwconv_train_fwd"] == (ctypes.c_int, [vp, i32, i32, i32, vp, i32, vp, vp, vp])
    assert sigs["ts_conformer_bn_stats"] == (ctypes.c_int, [vp, i32, i32, i32, f32, vp, vp, vp])
    assert sigs["ts_conformer_bn_act_cast"] == (ctypes.c_int, [vp, vp, vp, vp, i64, i32, i32, vp, vp, i64, i64, vp])
    assert sigs["ts_conformer_bn_act_bwd_sums_workspace"] == (i64, [i64, i32])
    assert sigs["ts_conformer_bn_act_bwd_sums"] == (ctypes.c_int, [vp, vp, vp, vp, vp, i64, i32, i32, vp, vp, vp, vp])
    assert sigs["ts_conformer_glu_dwconv_train_bwd_workspace"] == (i64, [i32, i32, i32, i32])
    assert sigs["ts_conformer_glu_dwconv_train_bwd"] == (ctypes.c_int, [vp, vp, vp, i32, i32, i32, vp, i32, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp])
    assert sigs["ts_conformer_rotary_bwd"] == (ctypes.c_int, [vp, vp, i32, i32, i32, vp, i32, vp, vp])
    assert sigs["ts_conformer_ffn_act_cast"] == (ctypes.c_int, [vp, vp, i64, i32, i32, f32, u64, vp, vp, i64, i64, vp])
    assert sigs["ts_conformer_ffn_act_bwd"] == (ctypes.c_int, [vp, vp, i32, i32, vp, f32, u64, vp, i64, vp])


def test_no_name_is_declared_in_two_headers_and_the_core_abi_is_unchanged():
    from thunder_speech_amd import _lib
    tables = (_lib.SIGNATURES, _lib.WAVLM_SIGNATURES, _lib.WAVLM_TRAIN_SIGNATURES, _lib.CONFORMER_SIGNATURES, _lib.MMS_SIGNATURES,
              _lib.MMS_TRAIN_SIGNATURES, _lib.MMS_ADAPTER_TRAIN_SIGNATURES, _lib.POSCONV_STACK_TRAIN_SIGNATURES, _lib.SEW_SIGNATURES,
              _lib.CTC_ALIGN_SIGNATURES, _lib.CTC_BEAM_SIGNATURES)
    for table in tables:
        assert not set(table) & set(NAMES)
    headers = glob.glob(os.path.join(ROOT, "include", "**", "*.h"), recursive=True) + glob.glob(os.path.join(ROOT, "thunder_speech_amd", "abi", "*.h"))
    assert len(headers) == 12 and HEADER in headers               # the core header and eleven companions
    seen = {}
    for path in headers:
        for name in _declared(path):
            assert name not in seen, f"{name}: declared in {seen[name]} and in {path}"
            seen[name] = path
    assert len(glob.glob(os.path.join(ROOT, "include", "*.h"))) == 7            # include/ keeps its file count
    assert len(_declared(os.path.join(ROOT, "include", "thunder_speech_amd.h"))) == 123 and _lib.ABI_VERSION == 15
    assert len(_lib.SIGNATURES) == len(_lib.EXPORTED_SYMBOLS) == 123


def test_built_library_defines_the_symbols_and_the_source_has_no_atomics_or_assembly():
    from thunder_speech_amd import build as b
    path = b.build(verbose=False)
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    assert set(NAMES) <= {line.split()[-1] for line in nm.splitlines() if line.strip()}
    src = open(os.path.join(ROOT, "thunder_speech_amd", "csrc", "conformer_train.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert '#include "conformer_train.h"' in src and "atomic" not in code and not re.search(r"\basm\b", code)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
transformers = pytest.importorskip("transformers")


def _adapt(train_precision="bf16", **over):
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    kw = dict(vocab_size=32, hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256, conv_dim=(32, 32, 32),
              conv_stride=(5, 2, 2), conv_kernel=(10, 3, 2), position_embeddings_type="rotary", conv_depthwise_kernel_size=5)
    model = transformers.Wav2Vec2ConformerModel(transformers.Wav2Vec2ConformerConfig(**{**kw, **over}))
    return HuggingFaceEncoderAdapt(model, train_precision=train_precision).train()


def _call(enc):
    return enc(torch.zeros(1, 4000), torch.tensor([4000]))                     # CPU tensors


def test_fp32_training_is_refused_by_name_and_names_the_way_in():
    enc = _adapt("fp32")
    with pytest.raises(NotImplementedError, match=r"wav2vec2-conformer.*train_precision='fp32'.*mixed precision only.*train_precision=\"bf16\""):
        _call(enc)


def test_mixed_precision_training_passes_the_refusals_and_reaches_the_gpu_check():
    with pytest.raises(RuntimeError, match="MI355X"):
        _call(_adapt("bf16"))


@pytest.mark.parametrize("kw,pattern", [(dict(add_adapter=True), r"wav2vec2-conformer.*add_adapter=True"),
                                        (dict(mask_feature_prob=0.1), r"wav2vec2-conformer.*mask_feature_prob"),
                                        (dict(intermediate_size=200), r"wav2vec2-conformer.*intermediate_size=200")])
def test_unsupported_training_configurations_are_refused_by_name_before_any_device_work(kw, pattern):
    with pytest.raises(NotImplementedError, match=pattern):
        _call(_adapt("bf16", **kw))


def test_mask_feature_prob_without_spec_augment_is_accepted():
    with pytest.raises(RuntimeError, match="MI355X"):
        _call(_adapt("bf16", mask_feature_prob=0.1, apply_spec_augment=False))


def test_an_unfrozen_feature_extractor_is_refused_by_name():
    enc = _adapt("bf16")
    next(enc.original_encoder.feature_extractor.parameters()).requires_grad_(True)
    with pytest.raises(NotImplementedError, match=r"wav2vec2-conformer.*feature extractor is frozen.*1 of its parameters"):
        _call(enc)


def test_the_unfused_attention_switch_is_refused_by_name(monkeypatch):
    from thunder_speech_amd.huggingface import train as T
    monkeypatch.setattr(T, "FUSED_ATTENTION", False)
    with pytest.raises(NotImplementedError, match=r"wav2vec2-conformer.*fused attention"):
        _call(_adapt("bf16"))


def test_the_wav2vec2_chain_still_does_not_list_the_conformer_and_sew_stays_refused():
    from thunder_speech_amd.huggingface import conformer_train as CT, train as T
    assert T.TRAINABLE_MODEL_TYPES == ("wav2vec2", "wavlm", "hubert", "unispeech", "unispeech-sat", "data2vec-audio")
    assert CT.refuse_untrainable is not T.refuse_untrainable
    with pytest.raises(NotImplementedError, match="inference-only"):
        T.refuse_untrainable(_adapt("bf16"), True)                              # train.py's own refusal is as it was
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    sew = transformers.SEWModel(transformers.SEWConfig(hidden_size=64, num_hidden_layers=1, num_attention_heads=2, intermediate_size=128,
                                                       conv_dim=(32, 32, 32), conv_stride=(5, 2, 2), conv_kernel=(10, 3, 2),
                                                       num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, squeeze_factor=2))
    with pytest.raises(NotImplementedError, match="sew"):
        HuggingFaceEncoderAdapt(sew, train_precision="bf16").train()(torch.zeros(1, 4000), torch.tensor([4000]))


def test_ffn_act_linear_keeps_its_six_argument_form():
    """The wav2vec2 chain calls FFNActLinear.apply with six arguments; the conformer chain appends the act code."""
    import inspect
    from thunder_speech_amd.huggingface import train as T
    params = list(inspect.signature(T.FFNActLinear.forward).parameters.values())
    assert [p.name for p in params] == ["ctx", "z", "b1", "w2", "b2", "p_drop", "seed", "act"] and params[-1].default == 1
