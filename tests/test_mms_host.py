"""MMS on the CPU (the companion C header: tests/test_abi_headers_host.py): which adapter configurations are accepted or refused (by name),
the refusal of fine-tuning, and load_huggingface_checkpoint(dir, target_lang=...) on a two-language directory."""
import json
import os

import pytest
import torch

transformers = pytest.importorskip("transformers")

BASE = ["<pad>", "<s>", "</s>", "<unk>", "|"]
VOCABS = {"aaa": BASE + list("abcdefghijklmnopqrstuvwxyz'"), "bbb": BASE + list("zyxwvutsrq")}
CFG = dict(hidden_size=160, num_hidden_layers=2, num_attention_heads=2, intermediate_size=320, feat_extract_norm="layer", conv_bias=True,
           do_stable_layer_norm=True, vocab_size=len(VOCABS["aaa"]), conv_dim=(32,) * 7, conv_kernel=(10, 3, 3, 3, 3, 2, 2),
           conv_stride=(5, 2, 2, 2, 2, 2, 2), num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, pad_token_id=0, adapter_attn_dim=16)


def _model(**kw):
    return transformers.Wav2Vec2Model(transformers.Wav2Vec2Config(**{**CFG, **kw}))


# ---- configurations ------------------------------------------------------------------------------------------------------------------------
def test_pre_ln_adapters_are_accepted_and_the_plan_packs_their_weights():
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt, Wav2Vec2Plan, has_attn_adapters
    model = _model()
    enc = HuggingFaceEncoderAdapt(model)
    assert has_attn_adapters(model.config)
    assert "original_encoder.encoder.layers.1.adapter_layer.linear_2.weight" in enc.state_dict()
    plan = Wav2Vec2Plan(model.config, model.state_dict(), "cpu", "fp32")        # packing needs no GPU
    want = [f"encoder.layers.{i}.adapter_layer.{k}" for i in range(2)
            for k in ("norm.weight", "norm.bias", "linear_1.weight", "linear_1.bias", "linear_2.weight", "linear_2.bias")]
    assert plan.attn_adapter_keys == want and set(want) == {k for k in model.state_dict() if "adapter_layer" in k}
    for i, lw in enumerate(plan.layers):
        assert lw["ad"]["w1"].shape == (16, 160) and lw["ad"]["w2"].shape == (160, 16)
        assert torch.equal(lw["ad"]["b2"], model.state_dict()[f"encoder.layers.{i}.adapter_layer.linear_2.bias"])
    assert not plan.mms_attention                                                 # fp32 mode keeps ts_w2v_attention_fwd
    assert Wav2Vec2Plan(model.config, model.state_dict(), "cpu", "bf16").mms_attention
    assert Wav2Vec2Plan(model.config, model.state_dict(), "cpu", "bf16").layers[0]["ad"]["w1"].dtype == torch.bfloat16


def test_a_model_without_adapters_packs_none():
    from thunder_speech_amd.huggingface.encoder import Wav2Vec2Plan, has_attn_adapters
    model = _model(adapter_attn_dim=None, num_attention_heads=4)
    plan = Wav2Vec2Plan(model.config, model.state_dict(), "cpu", "bf16")
    assert plan.attn_adapter_keys == [] and all("ad" not in lw for lw in plan.layers) and not plan.mms_attention      # head_dim 40
    # transformers' post-LN layer has no adapter whatever the config says: no keys, nothing refused, not even a dimension the kernel lacks
    post = _model(do_stable_layer_norm=False, adapter_attn_dim=24)
    assert not any("adapter_layer" in k for k in post.state_dict()) and not has_attn_adapters(post.config)
    assert Wav2Vec2Plan(post.config, post.state_dict(), "cpu", "fp32").attn_adapter_keys == []


@pytest.mark.parametrize("dim", [24, 8, 80])
def test_an_adapter_dimension_the_kernel_lacks_is_refused_by_name(dim):
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    with pytest.raises(NotImplementedError, match=rf"adapter_attn_dim={dim}\b"):
        HuggingFaceEncoderAdapt(_model(adapter_attn_dim=dim))


def test_training_mode_with_adapters_is_refused_by_name_before_any_device_work():
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    for train_precision in ("fp32", "bf16"):
        enc = HuggingFaceEncoderAdapt(_model(), train_precision=train_precision)
        enc.train()
        with pytest.raises(NotImplementedError, match="adapter_attn_dim"):
            enc(torch.zeros(1, 4000), torch.tensor([4000]))               # CPU tensors: the refusal comes before the GPU check
        enc.eval()
        with pytest.raises(RuntimeError):                                  # eval mode reaches the GPU check (no CPU path)
            enc(torch.zeros(1, 4000), torch.tensor([4000]))
    # without adapters training mode goes on to the GPU check as before
    enc = HuggingFaceEncoderAdapt(_model(adapter_attn_dim=None))
    enc.train()
    with pytest.raises(RuntimeError) as e:
        enc(torch.zeros(1, 4000), torch.tensor([4000]))
    assert not isinstance(e.value, NotImplementedError)


# ---- a two-language checkpoint directory through the loader ------------------------------------------------------------------------------
def _two_language_checkpoint(d):
    """What an MMS repository holds: the model saved with the first language's head, adapter.<lang>.safetensors per language (attention adapters
    + lm_head, the keys of _get_adapters()), a vocab.json nested by language.  -> {lang: adapter state dict}."""
    from safetensors.torch import save_file
    torch.manual_seed(21)
    transformers.Wav2Vec2ForCTC(transformers.Wav2Vec2Config(**CFG)).eval().save_pretrained(d)
    adapters = {}
    for lang, toks in VOCABS.items():
        shapes = transformers.Wav2Vec2ForCTC(transformers.Wav2Vec2Config(**{**CFG, "vocab_size": len(toks)}))._get_adapters()
        adapters[lang] = {k: torch.randn_like(v).contiguous() for k, v in shapes.items()}
        save_file(adapters[lang], os.path.join(d, f"adapter.{lang}.safetensors"))
    with open(os.path.join(d, "vocab.json"), "w") as f:
        json.dump({lang: {tok: i for i, tok in enumerate(toks)} for lang, toks in VOCABS.items()}, f)
    transformers.Wav2Vec2CTCTokenizer(os.path.join(d, "vocab.json"), target_lang="aaa").save_pretrained(d)
    transformers.Wav2Vec2FeatureExtractor(return_attention_mask=True).save_pretrained(d)
    return adapters


def test_target_lang_selects_the_language_of_a_two_language_directory(tmp_path, monkeypatch):
    from thunder_speech_amd.huggingface.compatibility import load_huggingface_checkpoint
    monkeypatch.setenv("HF_HUB_OFFLINE", "1")
    d = str(tmp_path / "mms")
    os.makedirs(d)
    adapters = _two_language_checkpoint(d)
    m = load_huggingface_checkpoint(d, target_lang="bbb")
    n = len(VOCABS["bbb"])
    assert n != len(VOCABS["aaa"])
    assert m.decoder[2].weight.shape == (n, 160) and m.encoder_final_dimension == 160
    assert torch.equal(m.decoder[2].weight, adapters["bbb"]["lm_head.weight"]) and torch.equal(m.decoder[2].bias, adapters["bbb"]["lm_head.bias"])
    assert m.text_transform.num_tokens == n
    assert list(m.text_transform.vocab.itos)[:n] == [" " if t == "|" else t for t in VOCABS["bbb"]]
    enc = m.encoder.original_encoder
    for i in range(2):
        assert torch.equal(enc.encoder.layers[i].adapter_layer.linear_1.weight,
                           adapters["bbb"][f"wav2vec2.encoder.layers.{i}.adapter_layer.linear_1.weight"])
    assert m.encoder.mask_input and not m.training
    # without target_lang nothing changes: the saved head, the tokenizer's own default language
    m0 = load_huggingface_checkpoint(d)
    assert m0.decoder[2].weight.shape == (len(VOCABS["aaa"]), 160) and m0.text_transform.num_tokens == len(VOCABS["aaa"])
    assert not torch.equal(m0.encoder.original_encoder.encoder.layers[0].adapter_layer.linear_1.weight,
                           adapters["bbb"]["wav2vec2.encoder.layers.0.adapter_layer.linear_1.weight"])
