"""wav2vec2-conformer fine-tuning on the CPU (the companion C header: tests/test_abi_headers_host.py): what the source may not hold, and the
refusals of huggingface/conformer_train.py, each by name and before any device work (CPU tensors: a refusal that came later would be the GPU
check's RuntimeError instead)."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_source_has_no_atomics_or_assembly():
    src = open(os.path.join(ROOT, "thunder_speech_amd", "csrc", "conformer_train.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert '#include "thunder_speech_amd/conformer_train.h"' in src and "atomic" not in code and not re.search(r"\basm\b", code)


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
