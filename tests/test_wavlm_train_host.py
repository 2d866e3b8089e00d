"""WavLM fine-tuning on the CPU (the companion C header: tests/test_abi_headers_host.py): a mixed-precision WavLM adapter in train mode gets
past the refusal to the GPU check, and what stays refused is refused by name before any device work."""
import pytest
import torch

transformers = pytest.importorskip("transformers")

CFG = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, vocab_size=32, conv_dim=(32,) * 7,
           conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_stride=(5, 2, 2, 2, 2, 2, 2), num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4)
FAMILIES = {"base": dict(feat_extract_norm="group", do_stable_layer_norm=False),
            "large": dict(feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True)}


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
