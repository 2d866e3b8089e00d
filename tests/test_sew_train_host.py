"""SEW fine-tuning on the CPU (the companion C header: tests/test_abi_headers_host.py): the
argument checks of its launchers (made-up pointers: none of these calls reaches a launch), the Python mirror of the support matrix against the
launchers' own geometry check, the refusals by name of huggingface/sew_train.py (CPU tensors reach them), and the data gradient's tap packing against
a float64 loop."""
import pytest
import torch

transformers = pytest.importorskip("transformers")

CFG = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, vocab_size=32, conv_dim=(32, 32, 64),
           conv_kernel=(10, 3, 2), conv_stride=(5, 2, 2), num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, squeeze_factor=2)


def _adapter(train_precision="bf16", **kw):
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    enc = HuggingFaceEncoderAdapt(transformers.SEWModel(transformers.SEWConfig(**{**CFG, **kw})), train_precision=train_precision)
    return enc.train()


# ---- argument checks ---------------------------------------------------------------------------------------------------------------------------
def _host_cases():
    """(entry point, arguments, expected status) of calls that return before any launch.  Pointers are made-up addresses (never dereferenced on these
    paths): A is 16-byte aligned, A + 4 / A + 2 are not.  Every call carries at least one argument that is refused."""
    A, E, U = 0x10000, -1, -2
    fw = lambda x=A, b=1, t=8, c=128, w=A, bias=A, k=4, groups=4, s=2, y=A, z=A, ws=A: (
        "ts_sew_squeeze_train_fwd", (x, b, t, c, w, bias, k, groups, s, y, z, ws, None))
    dg = lambda dz=A, dy=A, b=1, t=8, c=128, w=A, k=4, groups=4, s=2, dx=A, ws=A: ("ts_sew_squeeze_dgrad", (dz, dy, b, t, c, w, k, groups, s, dx, ws, None))
    wg = lambda dz=A, x=A, b=1, t=8, c=128, k=4, groups=4, s=2, dw=A, ws=A: ("ts_sew_squeeze_wgrad", (dz, x, b, t, c, k, groups, s, dw, ws, None))
    cases = [(fw(x=0), E), (fw(w=0), E), (fw(bias=0), E), (fw(y=0), E), (fw(z=0), E), (fw(ws=0), E),
             (fw(x=A + 4), U), (fw(w=A + 4), U), (fw(y=A + 4), U), (fw(z=A + 8), U), (fw(ws=A + 8), U), (fw(bias=A + 2), U),
             (dg(dz=0), E), (dg(dy=0), E), (dg(w=0), E), (dg(dx=0), E), (dg(ws=0), E),
             (dg(dz=A + 4), U), (dg(dy=A + 4), U), (dg(w=A + 8), U), (dg(dx=A + 4), U), (dg(ws=A + 8), U),
             (wg(dz=0), E), (wg(x=0), E), (wg(dw=0), E), (wg(ws=0), E),
             (wg(dz=A + 4), U), (wg(x=A + 4), U), (wg(dw=A + 8), U), (wg(ws=A + 8), U)]
    for f in (fw, dg, wg):
        cases += [(f(b=0), E), (f(t=0), E), (f(c=0), E), (f(k=0), E), (f(groups=0), E), (f(s=0), E), (f(s=-1), E), (f(t=2, s=3), E), (f(c=130), E),
                  (f(k=128, s=3), U), (f(c=96, k=400, s=1), U),                       # what ts_sew_squeeze_fwd(precision = 1) refuses: windows over 64 KiB
                  (f(c=256), U), (f(c=64), U), (f(c=192), U)]                         # 64, 16 and 48 channels per group
    for name in ("ts_sew_squeeze_dgrad_workspace_bytes", "ts_sew_squeeze_wgrad_workspace_bytes"):
        ws = lambda b=1, t=8, c=128, k=4, s=2: (name, (b, t, c, k, s))
        cases += [(ws(b=0), E), (ws(t=0), E), (ws(c=0), E), (ws(k=0), E), (ws(s=0), E), (ws(t=2, s=3), E)]
    return [(name, args, want) for (name, args), want in cases]


@pytest.mark.parametrize("name,args,want", _host_cases(), ids=lambda v: v if isinstance(v, str) else None)
def test_launchers_refuse_bad_arguments_before_any_launch(name, args, want):
    from thunder_speech_amd import _lib
    assert (_lib.TS_EINVAL, _lib.TS_EUNSUPPORTED) == (-1, -2)
    assert getattr(_lib.lib(), name)(*args) == want


def test_workspaces_hold_the_padded_bf16_copies():
    from thunder_speech_amd import _lib
    L = _lib.lib()
    for b, t, c, g, k, s in [(2, 261, 192, 8, 128, 2), (1, 7, 128, 4, 15, 3), (16, 999, 512, 16, 128, 2), (2, 5, 128, 4, 16, 1)]:
        t2, nt, prow = t // s, -(-k // s), -(-(t + k) // s) * s
        cp = g * 32
        assert L.ts_sew_squeeze_dgrad_workspace_bytes(b, t, c, k, s) >= b * (t2 + nt) * cp * 2
        assert L.ts_sew_squeeze_wgrad_workspace_bytes(b, t, c, k, s) >= b * (prow + t2) * cp * 2
        assert L.ts_sew_squeeze_dgrad_workspace_bytes(b, t, c, k, s) % 16 == 0 and L.ts_sew_squeeze_wgrad_workspace_bytes(b, t, c, k, s) % 16 == 0


@pytest.mark.parametrize("s", [1, 2, 3])
@pytest.mark.parametrize("k", [15, 16, 128])
@pytest.mark.parametrize("cg", [16, 24, 32, 64])
def test_support_mirror_equals_the_launchers_answer(cg, k, s):
    """squeeze_trains against ts_sew_squeeze_train_supported (the check all three launches make first), and -- for the refused geometries, where no
    launch can follow -- against the launches themselves; it is also the inference dispatch (squeeze_on_matrix_cores)."""
    from thunder_speech_amd import _lib
    from thunder_speech_amd.huggingface.sew import squeeze_on_matrix_cores
    from thunder_speech_amd.huggingface.sew_train import squeeze_trains
    L = _lib.lib()
    groups, A = 4, 0x10000
    c = cg * groups
    want = squeeze_trains(cg, k, s)
    assert want is squeeze_on_matrix_cores(cg, k, s)
    assert want is (cg in (24, 32) and not (k == 128 and s == 3))
    for b, t in [(1, 7), (2, 261)]:
        assert L.ts_sew_squeeze_train_supported(b, t, c, k, groups, s) == (0 if want else _lib.TS_EUNSUPPORTED)
    if not want:
        assert L.ts_sew_squeeze_train_fwd(A, 2, 261, c, A, A, k, groups, s, A, A, A, None) == _lib.TS_EUNSUPPORTED
        assert L.ts_sew_squeeze_dgrad(A, A, 2, 261, c, A, k, groups, s, A, A, None) == _lib.TS_EUNSUPPORTED
        assert L.ts_sew_squeeze_wgrad(A, A, 2, 261, c, k, groups, s, A, A, None) == _lib.TS_EUNSUPPORTED
        if cg in (24, 32):
            assert L.ts_sew_squeeze_fwd(A, 2, 261, c, A, A, k, groups, s, 1, A, A, None) == _lib.TS_EUNSUPPORTED


# ---- refusals by name --------------------------------------------------------------------------------------------------------------------------
X, N = torch.zeros(1, 4000), torch.tensor([4000])               # CPU tensors: every refusal comes before the GPU check


def test_fp32_fine_tuning_is_refused_by_name():
    enc = _adapter("fp32")
    with pytest.raises(NotImplementedError, match="sew: fine-tuning is not implemented") as e:
        enc(X, N)
    assert "train_precision='fp32'" in str(e.value) and 'train_precision="bf16"' in str(e.value)


def test_mixed_precision_training_reaches_the_gpu_check():
    enc = _adapter("bf16")
    with pytest.raises(RuntimeError) as e:
        enc(X, N)
    assert not isinstance(e.value, NotImplementedError), e.value


def test_64_channels_per_group_are_refused_by_name():
    enc = _adapter(num_conv_pos_embedding_groups=2)
    with pytest.raises(NotImplementedError, match=r"sew fine-tuning: 64 channels per group with num_conv_pos_embeddings=16 and squeeze_factor=2") as e:
        enc(X, N)
    assert "24 or 32 channels per group train" in str(e.value)


def test_a_window_over_the_lds_limit_is_refused_by_name():
    enc = _adapter(num_conv_pos_embeddings=128, squeeze_factor=3)
    with pytest.raises(NotImplementedError, match=r"sew fine-tuning: 32 channels per group with num_conv_pos_embeddings=128 and squeeze_factor=3"):
        enc(X, N)


def test_mask_feature_prob_is_refused_by_name():
    enc = _adapter(mask_feature_prob=0.1)
    with pytest.raises(NotImplementedError, match="sew fine-tuning: mask_feature_prob > 0 is not supported"):
        enc(X, N)
    _adapter(mask_feature_prob=0.1, apply_spec_augment=False)      # (without spec augment the probability is never read)
    with pytest.raises(RuntimeError) as e:
        _adapter(mask_feature_prob=0.1, apply_spec_augment=False)(X, N)
    assert not isinstance(e.value, NotImplementedError)


def test_an_unfrozen_feature_extractor_is_refused_by_name():
    enc = _adapter()
    next(enc.original_encoder.feature_extractor.parameters()).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="sew fine-tuning: the conv feature extractor is frozen") as e:
        enc(X, N)
    assert "1 of its parameters" in str(e.value)


def test_the_fused_attention_switch_is_refused_by_name(monkeypatch):
    from thunder_speech_amd.huggingface import train as T
    monkeypatch.setattr(T, "FUSED_ATTENTION", False)
    with pytest.raises(NotImplementedError, match="sew: fine-tuning runs on the fused attention only"):
        _adapter()(X, N)


def test_the_wav2vec2_chain_still_does_not_list_sew():
    from thunder_speech_amd.huggingface import train as T
    assert T.TRAINABLE_MODEL_TYPES == ("wav2vec2", "wavlm", "hubert", "unispeech", "unispeech-sat", "data2vec-audio")
    with pytest.raises(NotImplementedError, match="model_type='sew' is inference-only"):
        T.refuse_untrainable(_adapter(), True)


# ---- the data gradient's tap packing -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cg", [24, 32])
@pytest.mark.parametrize("k", [15, 16])
@pytest.mark.parametrize("s", [1, 2, 3])
def test_dgrad_tap_packing_gives_the_transposed_conv_in_a_float64_loop(s, k, cg):
    """Packed blocks, read the way the kernel reads them -- out_f[m] = sum_u dzp[m + u] Wd[f][u] over dz behind nt - 1 zero rows, row q = s m + f - p --
    against the data gradient written straight from its definition, both in float64 on the bf16-rounded weights."""
    from thunder_speech_amd.huggingface.sew_train import pack_squeeze_dgrad_taps
    groups, t = 2, 11
    g = torch.Generator().manual_seed(100 * s + 10 * k + cg)
    wk = torch.randn(k, groups, cg, cg, generator=g)
    packed = pack_squeeze_dgrad_taps(wk, s)
    nt, p, t2 = -(-k // s), k // 2, t // s
    assert packed.shape == (s, nt, groups, 32, 32) and packed.dtype == torch.bfloat16 and packed.is_contiguous()
    assert not bool(packed[..., cg:, :].any()) and not bool(packed[..., :, cg:].any())
    w16 = wk.to(torch.bfloat16).double()
    dz = torch.randn(t2, groups, cg, generator=g).double()
    want = torch.zeros(t, groups, cg, dtype=torch.float64)
    for q in range(t):
        for j in range(k):
            if (q + p - j) % s == 0 and 0 <= (q + p - j) // s < t2:
                want[q] += torch.einsum("go,goi->gi", dz[(q + p - j) // s], w16[j])
    dzp = torch.zeros(t2 + 2 * nt + t, groups, 32, dtype=torch.float64)
    dzp[nt - 1:nt - 1 + t2, :, :cg] = dz
    got = torch.full((t, groups, cg), float("nan"), dtype=torch.float64)
    for f in range(s):
        for m in range((t - 1 + p) // s + 1):
            q = s * m + f - p
            if 0 <= q < t:
                acc = sum(torch.einsum("go,gio->gi", dzp[m + u], packed[f, u].double()) for u in range(nt))
                got[q] = acc[:, :cg]
    assert not bool(torch.isnan(got).any())
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
