"""SEW on the CPU: which configurations are accepted or refused (each refusal by name, sew-d included), the refusal of fine-tuning, the pooled key
lengths against max_pool1d of transformers' mask, the tap packing, and the argument checks of the two launchers (made-up pointers: none of
these calls reaches a launch).  (The companion C header: tests/test_abi_headers_host.py.)"""
import pytest
import torch

transformers = pytest.importorskip("transformers")

CFG = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, vocab_size=32, conv_dim=(32, 32, 32, 32, 64),
           conv_kernel=(10, 3, 1, 3, 1), conv_stride=(5, 2, 1, 2, 1), num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, squeeze_factor=2)


def _config(**kw):
    return transformers.SEWConfig(**{**CFG, **kw})


def _model(**kw):
    return transformers.SEWModel(_config(**kw))


class _Stub(torch.nn.Module):
    """Only a config: what the adapter's configuration check reads (for configurations transformers itself cannot build a module from)."""

    def __init__(self, cfg):
        super().__init__()
        self.config = cfg


# ---- accepted and refused ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("taps", [16, 15])
@pytest.mark.parametrize("squeeze", [1, 2, 3])
@pytest.mark.parametrize("projection", [True, False])
@pytest.mark.parametrize("norm", ["group", "layer"])
def test_sew_is_accepted(norm, projection, squeeze, taps):
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt, SUPPORTED_MODEL_TYPES
    assert "sew" in SUPPORTED_MODEL_TYPES
    dims = CFG["conv_dim"] if projection else (32, 32, 32, 32, 128)
    enc = HuggingFaceEncoderAdapt(_model(feat_extract_norm=norm, conv_bias=norm == "layer", conv_dim=dims, squeeze_factor=squeeze,
                                         num_conv_pos_embeddings=taps))
    sd = enc.state_dict()
    assert "original_encoder.encoder.upsample.projection.weight" in sd and "original_encoder.layer_norm.weight" in sd
    assert ("original_encoder.feature_projection.weight" in sd) == projection
    assert sd["original_encoder.encoder.upsample.projection.weight"].shape == (128 * squeeze, 128)
    assert not any(p.requires_grad for p in enc.original_encoder.feature_extractor.parameters())


@pytest.mark.parametrize("kw,pattern", [(dict(num_attention_heads=4), r"model_type='sew' with head_dim=32"),
                                        (dict(hidden_act="relu"), r"model_type='sew' with hidden_act='relu'"),
                                        (dict(feat_extract_activation="relu"), r"model_type='sew' with feat_extract_activation='relu'"),
                                        (dict(squeeze_factor=0), r"model_type='sew' with squeeze_factor=0"),
                                        (dict(hidden_size=192, num_attention_heads=3, num_conv_pos_embedding_groups=5),
                                         r"model_type='sew' with hidden_size=192 not a multiple of num_conv_pos_embedding_groups=5"),
                                        (dict(add_adapter=True), r"model_type='sew' with add_adapter=True")])
def test_unsupported_sew_configurations_are_refused_by_name(kw, pattern):
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    with pytest.raises(NotImplementedError, match=pattern) as e:
        HuggingFaceEncoderAdapt(_Stub(_config(**kw)))
    assert str(e.value).startswith("sew HIP path: unsupported configuration")


def test_sew_d_is_still_refused_and_the_message_names_its_attention():
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt, SUPPORTED_MODEL_TYPES
    assert "sew-d" not in SUPPORTED_MODEL_TYPES
    with pytest.raises(NotImplementedError, match=r"model_type='sew-d' \(its disentangled attention has no HIP kernel"):
        HuggingFaceEncoderAdapt(_Stub(transformers.SEWDConfig()))


def test_sew_training_mode_is_refused_by_name_before_any_device_work():
    from thunder_speech_amd.huggingface import train as T
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    assert "sew" not in T.TRAINABLE_MODEL_TYPES
    enc = HuggingFaceEncoderAdapt(_model())
    enc.train()
    with pytest.raises(NotImplementedError, match="sew: fine-tuning is not implemented"):
        enc(torch.zeros(1, 4000), torch.tensor([4000]))               # CPU tensors: the refusal comes before the GPU check
    with pytest.raises(NotImplementedError, match="model_type='sew' is inference-only"):
        T.refuse_untrainable(enc, False)
    enc.eval()
    with pytest.raises(RuntimeError) as e:                             # eval mode reaches the GPU check (no CPU path)
        enc(torch.zeros(1, 4000), torch.tensor([4000]))
    assert not isinstance(e.value, NotImplementedError), e.value


def test_module_from_huggingface_builds_a_sew_ctc_module():
    from thunder_speech_amd.huggingface.compatibility import module_from_huggingface
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt

    class FE:
        return_attention_mask = False

    model = transformers.SEWForCTC(_config())
    module = module_from_huggingface(model, FE())
    assert isinstance(module.encoder, HuggingFaceEncoderAdapt) and module.encoder.original_encoder is model.sew
    assert module.encoder_final_dimension == 128 and not module.training


# ---- host helpers ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 2, 3])
@pytest.mark.parametrize("t", ["s", 7, 260, 261])
def test_pooled_key_lengths_equal_the_max_pool_of_the_mask_for_every_length(t, s):
    from thunder_speech_amd.huggingface.sew import pooled_key_lengths
    t = s if t == "s" else t
    t2 = t // s
    lens = torch.arange(t + 1)
    mask = (torch.arange(t)[None, :] < lens[:, None])
    pooled = torch.nn.functional.max_pool1d(mask.float().unsqueeze(1), kernel_size=s, stride=s).squeeze(1).long()      # SEWEncoder.forward
    assert pooled.shape == (t + 1, t2)
    got = pooled_key_lengths(lens, s, t2)
    assert torch.equal(got, pooled.sum(1))
    assert torch.equal(pooled, (torch.arange(t2)[None, :] < got[:, None]).long())        # and the ones are a prefix: a key LENGTH says it all


@pytest.mark.parametrize("cg,k,s,want", [(32, 128, 2, True), (24, 128, 2, True), (32, 128, 1, True), (32, 16, 3, True), (32, 128, 3, False),
                                         (64, 128, 2, False), (48, 16, 2, False)])
def test_matrix_core_dispatch_mirror(cg, k, s, want):
    from thunder_speech_amd.huggingface.sew import squeeze_on_matrix_cores
    assert squeeze_on_matrix_cores(cg, k, s) is want


def test_tap_packing_pads_24_channel_groups_with_zeros():
    from thunder_speech_amd.huggingface.sew import pack_squeeze_taps
    g = torch.Generator().manual_seed(0)
    w = torch.randn(48, 24, 5, generator=g)                                     # two groups of 24
    f32 = pack_squeeze_taps(w, 2, False)
    assert f32.shape == (5, 2, 24, 24) and f32.dtype == torch.float32 and f32.is_contiguous()
    assert torch.equal(f32[3, 1, 7, 11], w[24 + 7, 11, 3])
    packed = pack_squeeze_taps(w, 2, True)
    assert packed.shape == (5, 2, 32, 32) and packed.dtype == torch.bfloat16 and packed.is_contiguous()
    assert torch.equal(packed[:, :, :24, :24], f32.to(torch.bfloat16))
    assert not bool(packed[:, :, 24:, :].any()) and not bool(packed[:, :, :, 24:].any())


# ---- argument checks ---------------------------------------------------------------------------------------------------------------------------
def _sew_host_cases():
    """(entry point, arguments, expected status) of calls that return before any launch.  Pointers are made-up addresses (never dereferenced on these
    paths): A is 16-byte aligned, A + 4 / A + 2 are not."""
    A, E, U = 0x10000, -1, -2
    sq = lambda x=A, b=1, t=8, c=128, w=A, bias=A, k=4, groups=4, s=2, prec=1, y=A, ws=A: (
        "ts_sew_squeeze_fwd", (x, b, t, c, w, bias, k, groups, s, prec, y, ws, None))
    un = lambda src=A, b=1, t2=4, t=9, c=128, s=2, dst=A: ("ts_sew_unsqueeze_rows", (src, b, t2, t, c, s, dst, None))
    wsb = lambda b=1, t=8, c=128, k=4, s=2, prec=1: ("ts_sew_squeeze_workspace_bytes", (b, t, c, k, s, prec))
    cases = [
        (sq(x=0), E), (sq(w=0), E), (sq(bias=0), E), (sq(y=0), E), (sq(ws=0), E),
        (sq(b=0), E), (sq(t=0), E), (sq(c=0), E), (sq(k=0), E), (sq(groups=0), E),
        (sq(s=0), E), (sq(s=-1), E), (sq(t=2, s=3), E), (sq(c=130), E),                                # t < stride; c % groups
        (sq(prec=2), U), (sq(prec=-1), U),
        (sq(x=A + 4), U), (sq(w=A + 4), U), (sq(y=A + 4), U), (sq(ws=A + 8), U), (sq(bias=A + 2), U),
        (sq(prec=0, x=A + 4), U), (sq(prec=0, c=256, ws=A + 4), U),
        (sq(k=128, s=3), U), (sq(c=96, k=400, s=1), U),                                                # windows over 64 KiB of LDS (32 and 24 channels per group)
        (un(src=0), E), (un(dst=0), E), (un(b=0), E), (un(t2=0), E), (un(c=0), E), (un(s=0), E), (un(t=7), E),      # t < stride t2
        (un(c=130), U), (un(src=A + 4), U), (un(dst=A + 8), U),
        (wsb(b=0), E), (wsb(t=0), E), (wsb(c=0), E), (wsb(k=0), E), (wsb(s=0), E), (wsb(t=2, s=3), E), (wsb(prec=2), U),
    ]
    return [(name, args, want) for (name, args), want in cases]


@pytest.mark.parametrize("name,args,want", _sew_host_cases(), ids=lambda v: v if isinstance(v, str) else None)
def test_sew_launchers_refuse_bad_arguments_before_any_launch(name, args, want):
    from thunder_speech_amd import _lib
    assert (_lib.TS_EINVAL, _lib.TS_EUNSUPPORTED) == (-1, -2)
    assert getattr(_lib.lib(), name)(*args) == want


def test_workspace_serves_both_paths():
    """The byte count is the f32 path's (conv result + padded f32 copy); the matrix-core path's bf16 copy at 32 channels per slot is smaller
    for either group width."""
    from thunder_speech_amd import _lib
    L = _lib.lib()
    assert L.ts_sew_abi_version() == 1
    for b, t, c, k, s in [(2, 261, 192, 128, 2), (1, 7, 128, 15, 3), (16, 999, 512, 128, 2)]:
        prow = -(-(t + k) // s) * s
        want = b * (prow // s + prow) * c * 4
        assert L.ts_sew_squeeze_workspace_bytes(b, t, c, k, s, 0) == want == L.ts_sew_squeeze_workspace_bytes(b, t, c, k, s, 1)
        assert b * prow * (c // 24) * 32 * 2 <= want
