"""WavLM fine-tuning on the CPU: the second companion header (include/thunder_speech_amd_wavlm_train.h) is bound and exported next to the
unchanged core and WavLM ABIs, a mixed-precision WavLM adapter in train mode gets past the refusal to the GPU check, and what stays refused is
refused by name before any device work."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

transformers = pytest.importorskip("transformers")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CFG = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, vocab_size=32, conv_dim=(32,) * 7,
           conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_stride=(5, 2, 2, 2, 2, 2, 2), num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4)
FAMILIES = {"base": dict(feat_extract_norm="group", do_stable_layer_norm=False),
            "large": dict(feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True)}


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ts_[a-z0-9_]+)\s*\(", src)))


def test_training_header_is_bound_exported_and_disjoint_from_the_other_two():
    from thunder_speech_amd import _lib, build as b
    train = _declared(os.path.join(ROOT, "include", "thunder_speech_amd_wavlm_train.h"))
    assert sorted(_lib.WAVLM_TRAIN_SIGNATURES) == train and _lib.WAVLM_TRAIN_ABI_VERSION == 1
    assert {"ts_wavlm_train_abi_version", "ts_wavlm_gate_fwd", "ts_wavlm_gate_bwd", "ts_wavlm_attention_train_fwd", "ts_wavlm_attention_train_bwd",
            "ts_wavlm_rel_bias_bwd"} <= set(train)
    wavlm = _declared(os.path.join(ROOT, "include", "thunder_speech_amd_wavlm.h"))
    core = _declared(os.path.join(ROOT, "include", "thunder_speech_amd.h"))
    assert not set(train) & set(wavlm) and not set(train) & set(core)
    # the other two ABIs are what they were
    assert len(core) == 123 and sorted(_lib.SIGNATURES) == core and _lib.EXPORTED_SYMBOLS == list(_lib.SIGNATURES) and _lib.ABI_VERSION == 15
    assert sorted(_lib.WAVLM_SIGNATURES) == wavlm and len(wavlm) == 4 and _lib.WAVLM_ABI_VERSION == 1
    vp, i32, i64, f32, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_uint64
    assert _lib.WAVLM_TRAIN_SIGNATURES["ts_wavlm_attention_train_bwd"][1] == [vp, i32, i32, i32, i32, vp, f32, u64] + [vp] * 11
    assert _lib.WAVLM_TRAIN_SIGNATURES["ts_wavlm_gate_fwd"][1] == [vp, i32, i32, i32, i64] + [vp] * 6
    assert _lib.WAVLM_TRAIN_SIGNATURES["ts_wavlm_attention_train_bwd_workspace"][0] == i64
    path = b.build(verbose=False)
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert not [s for s in train if s not in defined]


@pytest.mark.parametrize("family", list(FAMILIES))
def test_mixed_precision_wavlm_training_gets_past_the_refusal_to_the_gpu_check(family):
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    enc = HuggingFaceEncoderAdapt(transformers.WavLMModel(transformers.WavLMConfig(**{**CFG, **FAMILIES[family]})), train_precision="bf16")
    enc.train()
    with pytest.raises(RuntimeError) as err:
        enc(torch.zeros(1, 4000), torch.tensor([4000]))          # CPU tensors: the training path starts and stops at the GPU check
    assert not isinstance(err.value, NotImplementedError)


def test_fp32_wavlm_training_is_refused_by_name_and_points_at_bf16():
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    enc = HuggingFaceEncoderAdapt(transformers.WavLMModel(transformers.WavLMConfig(**{**CFG, **FAMILIES["base"]})))
    enc.train()
    with pytest.raises(NotImplementedError, match=r'wavlm.*train_precision="bf16"'):
        enc(torch.zeros(1, 4000), torch.tensor([4000]))


@pytest.mark.parametrize("over,what", [(dict(add_adapter=True, num_adapter_layers=1, output_hidden_size=64), "add_adapter"),
                                       (dict(mask_feature_prob=0.1), "mask_feature_prob")])
def test_untrainable_wavlm_configurations_stay_refused_by_name_before_any_device_work(over, what):
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    enc = HuggingFaceEncoderAdapt(transformers.WavLMModel(transformers.WavLMConfig(**{**CFG, **FAMILIES["base"], **over})), train_precision="bf16")
    enc.train()
    with pytest.raises(NotImplementedError, match=what):
        enc(torch.zeros(1, 4000), torch.tensor([4000]))


def test_unfrozen_feature_extractor_and_head_dim_16_stay_refused():
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    enc = HuggingFaceEncoderAdapt(transformers.WavLMModel(transformers.WavLMConfig(**{**CFG, **FAMILIES["large"]})), train_precision="bf16")
    next(enc.original_encoder.feature_extractor.parameters()).requires_grad_(True)
    enc.train()
    with pytest.raises(NotImplementedError, match="feature extractor is frozen"):
        enc(torch.zeros(1, 4000), torch.tensor([4000]))
    with pytest.raises(NotImplementedError, match=r"wavlm.*head_dim=16"):
        HuggingFaceEncoderAdapt(transformers.WavLMModel(transformers.WavLMConfig(**{**CFG, **FAMILIES["base"], "num_attention_heads": 8})),
                                train_precision="bf16")
