"""LoRA fine-tuning of the attention projections on the CPU (the companion C header: tests/test_abi_headers_host.py): that the entry points fail
loudly without a library, and the regime -- what HuggingFaceEncoderAdapt.lora_finetuning() sets up, merge_lora(), the LoRA-only state dict, and
which configurations are refused by name."""
import math

import pytest
import torch

NAMES = sorted(["ts_lora_abi_version", "ts_lora_fwd", "ts_lora_bwd_workspace", "ts_lora_bwd"])
# a tiny wav2vec2: hidden 128, 2 layers, 2 heads
CFG = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, vocab_size=32, conv_dim=(32, 32, 32),
           conv_kernel=(10, 3, 2), conv_stride=(5, 2, 2), num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=2, pad_token_id=0)


# ---- no library, no entry points ----------------------------------------------------------------------------------------------------------------
def test_without_a_library_the_entry_points_fail_loudly(monkeypatch, tmp_path):
    """The same path as every other entry point: lib() raises by name when the shared library is missing (no CPU fallback), and a library
    without the four symbols is refused at load."""
    from thunder_speech_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "lib_path", lambda: str(tmp_path / "libthunder_speech_hip.so"))
    for name in NAMES:
        with pytest.raises(RuntimeError, match="is missing"):
            getattr(_lib.lib(), name)
    assert set(NAMES) <= set(_lib.COMPANIONS["lora_train"].signatures)


# ---- the regime --------------------------------------------------------------------------------------------------------------------------------
def _adapt(train_precision="bf16", cls="Wav2Vec2", **kw):
    transformers = pytest.importorskip("transformers")
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    torch.manual_seed(0)
    model = getattr(transformers, cls + "Model")(getattr(transformers, cls + "Config")(**{**CFG, **kw}))
    return model, HuggingFaceEncoderAdapt(model, train_precision=train_precision)


def _train_forward_error(enc):
    enc.train()
    with pytest.raises(Exception) as e:
        enc(torch.zeros(1, 4000), torch.tensor([4000]))             # CPU tensors: a refusal by name comes first, else the GPU check (no CPU path)
    return e.value


@pytest.mark.parametrize("rank,targets", [(8, ("q_proj", "v_proj")), (16, ("q_proj", "k_proj", "v_proj", "out_proj")), (32, ("out_proj",))])
def test_lora_finetuning_freezes_the_base_and_registers_the_pairs(rank, targets):
    model, enc = _adapt()
    before = set(enc.state_dict())
    named = enc.lora_finetuning(rank=rank, alpha=2.0 * rank, targets=targets)
    assert enc.lora_scale == 2.0
    assert all(not p.requires_grad for p in model.parameters())
    assert set(named) == set(enc.state_dict()) - before
    assert set(named) == {f"lora.layers.{i}.{t}.lora_{m}" for i in range(2) for t in targets for m in "AB"}
    assert {n for n, p in enc.named_parameters() if p.requires_grad} == set(named)
    assert all(named[n] is p for n, p in enc.named_parameters() if n in named)
    for n, p in named.items():
        assert p.dtype == torch.float32 and p.requires_grad
        p = p.detach()
        if n.endswith("lora_A"):
            assert tuple(p.shape) == (rank, 128) and float(p.abs().max()) > 0 and float(p.abs().max()) <= 1.0 / math.sqrt(128) + 1e-6
        else:
            assert tuple(p.shape) == (128, rank) and float(p.abs().max()) == 0.0
    assert sum(p.numel() for p in named.values()) == 2 * len(targets) * rank * (128 + 128)
    with pytest.raises(RuntimeError, match="already"):
        enc.lora_finetuning()


def test_bad_rank_and_target_are_value_errors():
    _, enc = _adapt()
    for rank in (0, 4, 12, 128, 8.0, True):
        with pytest.raises(ValueError, match="rank"):
            enc.lora_finetuning(rank=rank)
    for targets in (("q_proj", "w_proj"), (), ("q_proj", "q_proj"), ("intermediate_dense",)):
        with pytest.raises(ValueError, match="targets"):
            enc.lora_finetuning(targets=targets)
    with pytest.raises(ValueError, match="alpha"):
        enc.lora_finetuning(alpha=0.0)
    assert not hasattr(enc, "lora") and any(p.requires_grad for p in enc.parameters())      # nothing happened


def test_merge_lora_adds_the_scaled_product_within_one_f32_rounding_and_removes_the_pairs():
    model, enc = _adapt()
    named = enc.lora_finetuning(rank=8, alpha=16.0, targets=("q_proj", "out_proj"))
    with torch.no_grad():
        for p in named.values():
            p.copy_(0.1 * torch.randn_like(p))
    w0 = {n: p.detach().clone() for n, p in model.named_parameters()}
    pairs = {n: p.detach().clone() for n, p in named.items()}
    enc.merge_lora()
    assert not hasattr(enc, "lora") and not any(k.startswith("lora.") for k in enc.state_dict())
    assert all(not p.requires_grad for p in enc.parameters())
    touched = set()
    for i in range(2):
        for t in ("q_proj", "out_proj"):
            key = f"encoder.layers.{i}.attention.{t}.weight"
            a, b = pairs[f"lora.layers.{i}.{t}.lora_A"].double(), pairs[f"lora.layers.{i}.{t}.lora_B"].double()
            want = w0[key].double() + 2.0 * (b @ a)
            got = dict(model.named_parameters())[key].detach().double()
            # one rounding of the f32 product (8 terms), one of the sum: 2^-23 of the largest magnitude each, and the f32 dot's own error
            assert float((got - want).abs().max()) <= 2.0 ** -21 * float(want.abs().max())
            assert float((got - w0[key].double()).abs().max()) > 1e-3
            touched.add(key)
    for n, p in model.named_parameters():
        if n not in touched:
            assert torch.equal(p.detach(), w0[n]), n
    with pytest.raises(RuntimeError, match="no LoRA"):
        enc.merge_lora()
    enc.lora_finetuning(rank=16)                                     # a second adaptation on the merged base


def test_lora_state_dict_round_trip_is_bit_equal():
    _, enc = _adapt()
    named = enc.lora_finetuning(rank=16, alpha=32.0, targets=("q_proj", "v_proj"))
    with torch.no_grad():
        for p in named.values():
            p.copy_(torch.randn_like(p))
    sd = enc.lora_state_dict()
    assert set(sd) == set(named) and all(torch.equal(sd[n], named[n].detach()) and sd[n].data_ptr() != named[n].data_ptr() for n in sd)
    _, other = _adapt()
    with pytest.raises(RuntimeError, match="lora_finetuning"):
        other.load_lora_state_dict(sd)
    theirs = other.lora_finetuning(rank=16, alpha=32.0, targets=("q_proj", "v_proj"))
    other.load_lora_state_dict(sd)
    assert all(torch.equal(theirs[n].detach(), sd[n]) for n in sd)
    assert all(torch.equal(v, sd[k]) for k, v in other.lora_state_dict().items())
    with pytest.raises(KeyError):
        other.load_lora_state_dict({k: v for k, v in sd.items() if "layers.0" in k})
    _, third = _adapt()
    third.lora_finetuning(rank=8, targets=("q_proj", "v_proj"))
    with pytest.raises(ValueError, match="shape"):
        third.load_lora_state_dict(sd)


# ---- refusals, by name, before any device work ---------------------------------------------------------------------------------------------------
def test_f32_training_with_lora_is_refused_by_name():
    _, enc = _adapt(train_precision="fp32")
    enc.lora_finetuning()
    err = _train_forward_error(enc)
    assert isinstance(err, NotImplementedError) and "LoRA" in str(err) and "train_precision='fp32'" in str(err) and 'train_precision="bf16"' in str(err)
    enc.train_precision = "bf16"
    err = _train_forward_error(enc)
    assert isinstance(err, RuntimeError) and not isinstance(err, NotImplementedError), err          # the GPU check is reached


def test_a_trainable_base_parameter_is_refused_by_name():
    model, enc = _adapt()
    enc.lora_finetuning()
    model.encoder.layers[1].attention.k_proj.weight.requires_grad_(True)
    err = _train_forward_error(enc)
    assert isinstance(err, NotImplementedError) and "frozen base" in str(err) and "encoder.layers.1.attention.k_proj.weight" in str(err)
    assert "lora_finetuning()" in str(err)
    enc.eval()                                                       # eval mode refuses nothing


def test_conformer_sew_and_mms_are_refused_by_name():
    transformers = pytest.importorskip("transformers")
    _, conf = _adapt(cls="Wav2Vec2Conformer", position_embeddings_type="rotary", conv_depthwise_kernel_size=7)
    with pytest.raises(NotImplementedError, match="LoRA on model_type='wav2vec2-conformer'"):
        conf.lora_finetuning()
    _, sew = _adapt(cls="SEW", hidden_size=128, num_attention_heads=2, squeeze_factor=2)
    with pytest.raises(NotImplementedError, match="LoRA on model_type='sew'"):
        sew.lora_finetuning()
    _, mms = _adapt(hidden_size=160, intermediate_size=320, num_conv_pos_embedding_groups=4, feat_extract_norm="layer", conv_bias=True,
                    do_stable_layer_norm=True, adapter_attn_dim=16)
    with pytest.raises(NotImplementedError, match="LoRA together with adapter_attn_dim=16"):
        mms.lora_finetuning()
    for enc in (conf, sew, mms):
        assert not hasattr(enc, "lora")
    # the same refusals guard the train-mode forward (a LoRA container that got there some other way)
    from thunder_speech_amd.huggingface import train as T
    _, plain = _adapt()
    plain.lora_finetuning()
    mms.lora, mms.lora_scale = plain.lora, plain.lora_scale
    err = _train_forward_error(mms)
    assert isinstance(err, NotImplementedError) and "adapter_attn_dim=16" in str(err) and "LoRA" in str(err)
    assert T.FUSED_ATTENTION is True                                 # (it has no bearing on any of these)


def test_configure_optimizers_holds_exactly_the_lora_tensors_and_the_decoder():
    from thunder_speech_amd.blocks import linear_decoder
    from thunder_speech_amd.huggingface.transform import Wav2Vec2Preprocess
    from thunder_speech_amd.module import BaseCTCModule
    from thunder_speech_amd.text_processing.transform import BatchTextTransformer
    _, enc = _adapt()
    tokens = [chr(97 + i) for i in range(26)] + [" "]
    module = BaseCTCModule(enc, linear_decoder(128, len(tokens) + 1, 0.0), Wav2Vec2Preprocess(), BatchTextTransformer(tokens=tokens))
    stamp0 = module._weights_stamp()
    named = enc.lora_finetuning(rank=8)
    opt = module.configure_optimizers()
    trained = {id(p) for group in opt.param_groups for p in group["params"]}
    assert trained == {id(p) for p in named.values()} | {id(p) for p in module.decoder.parameters()}
    # the inference-graph stamp follows the new parameters without a train() / eval() in between, and an in-place step on them
    stamp1 = module._weights_stamp()
    assert stamp1 != stamp0
    with torch.no_grad():
        next(iter(named.values())).add_(1.0)
    stamp2 = module._weights_stamp()
    assert stamp2 != stamp1
    enc.merge_lora()
    assert module._weights_stamp() != stamp2
