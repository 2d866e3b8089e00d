"""WavLM on the CPU: the host bucket table of the gated relative-position bias against transformers, which configurations are accepted or
refused, and the refusal of fine-tuning.  (The companion C header: tests/test_abi_headers_host.py.)"""
import pytest
import torch

transformers = pytest.importorskip("transformers")

CFG = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, vocab_size=32, conv_dim=(32,) * 7,
           conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_stride=(5, 2, 2, 2, 2, 2, 2), num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4)
FAMILIES = {"base": dict(feat_extract_norm="group", do_stable_layer_norm=False),
            "large": dict(feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True)}


@pytest.mark.parametrize("nb,md", [(320, 800), (32, 40), (64, 100)])
def test_bucket_table_reproduces_transformers_exactly(nb, md):
    from transformers.models.wavlm.modeling_wavlm import WavLMAttention
    from thunder_speech_amd.huggingface.encoder import relative_position_bucket, wavlm_bucket_table
    att = WavLMAttention(64, 1, num_buckets=nb, max_distance=md)
    d = torch.arange(-5000, 5001)
    want = att._relative_positions_bucket(d)
    table = wavlm_bucket_table(nb, md)
    assert table.dtype == torch.int32 and table.shape == (md + 1,)
    assert int(table.max()) == nb // 2 - 1 and int(table[md]) == nb // 2 - 1
    # what ts_wavlm_rel_bias computes on the device: sign offset + table lookup at min(|d|, max_distance)
    got = (d > 0).long() * (nb // 2) + table.long()[d.abs().clamp(max=md)]
    assert torch.equal(got, want)
    assert torch.equal(relative_position_bucket(d, nb, md), want)
    # the [t][t] form compute_bias evaluates
    rp = torch.arange(300)[None, :] - torch.arange(300)[:, None]
    assert torch.equal((rp > 0).long() * (nb // 2) + table.long()[rp.abs().clamp(max=md)], att._relative_positions_bucket(rp))


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("adapter", [False, True])
def test_head_dim_64_wavlm_is_accepted_and_head_dim_16_refused(family, adapter):
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt, SUPPORTED_MODEL_TYPES
    assert "wavlm" in SUPPORTED_MODEL_TYPES
    extra = dict(add_adapter=True, num_adapter_layers=1, output_hidden_size=64) if adapter else {}
    enc = HuggingFaceEncoderAdapt(transformers.WavLMModel(transformers.WavLMConfig(**{**CFG, **FAMILIES[family], **extra})))
    assert "original_encoder.encoder.layers.0.attention.rel_attn_embed.weight" in enc.state_dict()
    with pytest.raises(NotImplementedError, match=r"wavlm.*head_dim=16"):
        HuggingFaceEncoderAdapt(transformers.WavLMModel(transformers.WavLMConfig(**{**CFG, **FAMILIES[family], **extra, "num_attention_heads": 8})))


def test_wavlm_training_mode_is_refused_by_name_before_any_device_work():
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    enc = HuggingFaceEncoderAdapt(transformers.WavLMModel(transformers.WavLMConfig(**{**CFG, **FAMILIES["base"]})))
    enc.train()
    with pytest.raises(NotImplementedError, match="wavlm"):
        enc(torch.zeros(1, 4000), torch.tensor([4000]))          # CPU tensors: the refusal comes before the GPU check
    enc.eval()
    with pytest.raises(RuntimeError):                              # eval mode reaches the GPU check (no CPU path)
        enc(torch.zeros(1, 4000), torch.tensor([4000]))
