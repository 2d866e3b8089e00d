"""wav2vec2-conformer on the CPU: the host rotary table against transformers, which configurations are accepted or refused (each refusal by
name), and the refusal of fine-tuning.  (The companion C header: tests/test_abi_headers_host.py.)"""
import pytest
import torch

transformers = pytest.importorskip("transformers")

CFG = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, vocab_size=32, conv_dim=(32,) * 7,
           conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_stride=(5, 2, 2, 2, 2, 2, 2), num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4,
           position_embeddings_type="rotary", conv_depthwise_kernel_size=31)


def _model(**kw):
    return transformers.Wav2Vec2ConformerModel(transformers.Wav2Vec2ConformerConfig(**{**CFG, **kw}))


@pytest.mark.parametrize("t", [1, 75, 999, 1500])
def test_rotary_table_equals_transformers_bit_for_bit(t):
    from transformers.models.wav2vec2_conformer.modeling_wav2vec2_conformer import Wav2Vec2ConformerRotaryPositionalEmbedding
    from thunder_speech_amd.huggingface.conformer import rotary_table
    cfg = transformers.Wav2Vec2ConformerConfig(**{**CFG, "hidden_size": 1024, "num_attention_heads": 16})
    emb = Wav2Vec2ConformerRotaryPositionalEmbedding(cfg)
    want = emb(torch.zeros(1, t, 1024))                              # [2][t][1][1][64]
    assert want.shape == (2, t, 1, 1, 64)
    want = want[:, :, 0, 0, :]
    assert torch.equal(want[..., 32:], want[..., :32])               # transformers repeats the 32 frequencies
    table = rotary_table(emb.inv_freq, 5000)
    assert table.dtype == torch.float32 and table.shape == (2, 5000, 32)
    assert torch.equal(table[:, :t], want[..., :32])                 # the prefix of the long table IS the short one


def test_the_rotary_buffer_is_in_the_state_dict():
    sd = _model().state_dict()
    assert "encoder.embed_positions.inv_freq" in sd and sd["encoder.embed_positions.inv_freq"].shape == (32,)


@pytest.mark.parametrize("act", ["swish", "gelu"])
@pytest.mark.parametrize("norm", ["group", "layer"])
@pytest.mark.parametrize("adapter", [False, True])
def test_rotary_conformer_is_accepted(act, norm, adapter):
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt, SUPPORTED_MODEL_TYPES
    assert "wav2vec2-conformer" in SUPPORTED_MODEL_TYPES
    extra = dict(add_adapter=True, num_adapter_layers=1, output_hidden_size=64) if adapter else {}
    enc = HuggingFaceEncoderAdapt(_model(hidden_act=act, feat_extract_norm=norm, **extra))
    assert "original_encoder.encoder.layers.0.conv_module.depthwise_conv.weight" in enc.state_dict()


@pytest.mark.parametrize("kw,pattern", [(dict(position_embeddings_type="relative"), r"wav2vec2-conformer.*position_embeddings_type='relative'"),
                                        (dict(position_embeddings_type=None), r"wav2vec2-conformer.*position_embeddings_type=None"),
                                        (dict(num_attention_heads=4), r"wav2vec2-conformer.*head_dim=32"),
                                        (dict(hidden_act="relu"), r"wav2vec2-conformer.*hidden_act='relu'"),
                                        (dict(conv_depthwise_kernel_size=65), r"wav2vec2-conformer.*conv_depthwise_kernel_size=65")])
def test_unsupported_conformers_are_refused_by_name(kw, pattern):
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    with pytest.raises(NotImplementedError, match=pattern):
        HuggingFaceEncoderAdapt(_model(**kw))


def test_relative_and_none_get_messages_of_their_own():
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    msgs = []
    for pet in ("relative", None):
        with pytest.raises(NotImplementedError) as e:
            HuggingFaceEncoderAdapt(_model(position_embeddings_type=pet))
        msgs.append(str(e.value))
    assert "Transformer-XL" in msgs[0] and "Transformer-XL" not in msgs[1]


def test_conformer_training_mode_is_refused_by_name_before_any_device_work():
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    enc = HuggingFaceEncoderAdapt(_model())
    enc.train()
    with pytest.raises(NotImplementedError, match="wav2vec2-conformer"):
        enc(torch.zeros(1, 4000), torch.tensor([4000]))               # CPU tensors: the refusal comes before the GPU check
    enc.eval()
    with pytest.raises(RuntimeError):                                  # eval mode reaches the GPU check (no CPU path)
        enc(torch.zeros(1, 4000), torch.tensor([4000]))
