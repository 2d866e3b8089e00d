"""Adapter-only fine-tuning of MMS checkpoints on the CPU (the companion C header: tests/test_abi_headers_host.py): the regime -- which models
train mode refuses by name and what HuggingFaceEncoderAdapt.adapter_finetuning() sets up."""
import pytest
import torch

# tests/test_mms_host.py's model: hidden 160, 2 heads (head_dim 80), adapter 16
CFG = dict(hidden_size=160, num_hidden_layers=2, num_attention_heads=2, intermediate_size=320, feat_extract_norm="layer", conv_bias=True,
           do_stable_layer_norm=True, vocab_size=32, conv_dim=(32,) * 7, conv_kernel=(10, 3, 3, 3, 3, 2, 2),
           conv_stride=(5, 2, 2, 2, 2, 2, 2), num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, pad_token_id=0, adapter_attn_dim=16)


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
