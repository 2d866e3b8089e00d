"""Fine-tuning of HuBERT, UniSpeech, UniSpeech-SAT and data2vec-audio checkpoints on the CPU: train mode gets past the refusal by name to the GPU
check for every one of them, and what data2vec-audio still refuses (by name, with the wording the other families get).  (The companion C
header of data2vec-audio's positional stack: tests/test_abi_headers_host.py.)"""
import pytest
import torch

transformers = pytest.importorskip("transformers")

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


def test_mixed_precision_restores_the_mode_it_found_on_return_on_exception_and_when_nested():
    from thunder_speech_amd.huggingface import train as T
    assert T._MIXED is False
    with T.mixed_precision(True):
        assert T._MIXED is True
        with T.mixed_precision(False):
            assert T._MIXED is False
            with T.mixed_precision(True):
                assert T._MIXED is True
            assert T._MIXED is False
        assert T._MIXED is True                                # the inner block did not clear the outer one's mode
        with pytest.raises(KeyError):
            with T.mixed_precision(False):
                assert T._MIXED is False
                raise KeyError("out by exception")
        assert T._MIXED is True
    assert T._MIXED is False
    with pytest.raises(KeyError):
        with T.mixed_precision(True):
            raise KeyError("out by exception")
    assert T._MIXED is False


def test_every_supported_model_type_resolves_to_a_chain_module_with_the_two_entry_points():
    import inspect
    from thunder_speech_amd.huggingface import conformer_train, encoder, sew_train, train
    assert set(encoder.TRAIN_CHAINS) == set(encoder.SUPPORTED_MODEL_TYPES)
    for model_type in encoder.SUPPORTED_MODEL_TYPES:
        chain = encoder.train_chain(model_type)
        assert chain is {"wav2vec2-conformer": conformer_train, "sew": sew_train}.get(model_type, train), model_type
        params = list(inspect.signature(chain.train_forward).parameters)
        assert params == ["adapt", "audio", "lengths"], (model_type, params)
        required = [p for p in inspect.signature(chain.refuse_untrainable).parameters.values() if p.default is p.empty]
        assert [p.name for p in required] == ["adapt"], (model_type, required)           # callable with the adapter alone


def test_the_conformer_is_still_refused_by_name_in_both_places():
    from thunder_speech_amd.huggingface import train as T
    assert "wav2vec2-conformer" not in T.TRAINABLE_MODEL_TYPES
    assert set(T.TRAINABLE_MODEL_TYPES) == {"wav2vec2", "wavlm", "hubert", "unispeech", "unispeech-sat", "data2vec-audio"}
