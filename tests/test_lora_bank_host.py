"""The LoRA bank on the CPU: the queued header include_staged/thunder_speech_amd/queued/lora_bank.h through `_lib.QUEUED` and the built library's
symbols, COMPANIONS and STAGED untouched by it; the bank's bookkeeping on a tiny Wav2Vec2Model that never leaves the host (state_dict keys, add /
remove / names, the id buffer select_adapters fills); and every refusal, by name and before the GPU check."""
import ctypes
import glob
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, i32, i64, cint = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int

NAMES = ["ts_lora_bank_abi_version", "ts_lora_bank_fwd"]
SIGNATURES = {
    "ts_lora_bank_abi_version": (cint, []),
    "ts_lora_bank_fwd": (cint, [vp, i32, i64, i32, i32, i32, vp, vp, vp, i32, i32, i32, i32, vp, vp, i32, i64, i32, i32, i32, vp]),
}
# a tiny wav2vec2: hidden 128, 2 layers, 2 heads (tests/test_lora_host.py)
CFG = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, vocab_size=32, conv_dim=(32, 32, 32),
           conv_kernel=(10, 3, 2), conv_stride=(5, 2, 2), num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=2, pad_token_id=0)
QV, ALL = ("q_proj", "v_proj"), ("q_proj", "k_proj", "v_proj", "out_proj")


# ---- the binder ------------------------------------------------------------------------------------------------------------------------------
def test_queued_header_parses_and_declares_exactly_its_names():
    from thunder_speech_amd import _lib
    assert list(_lib.QUEUED) == ["lora_bank"]
    h = _lib.QUEUED["lora_bank"]
    assert h.path == os.path.join(ROOT, "include_staged", "thunder_speech_amd", "queued", "lora_bank.h")
    assert list(h.signatures) == NAMES and h.signatures == SIGNATURES
    assert (h.version_define, h.version_function, h.abi_version) == ("TS_LORA_BANK_ABI_VERSION", "ts_lora_bank_abi_version", 1)
    assert h.structs == {} and h.defines == {"TS_LORA_BANK_ABI_VERSION": 1}
    others = set(_lib.CORE.signatures).union(*(c.signatures for c in list(_lib.COMPANIONS.values()) + list(_lib.STAGED.values())))
    assert not others & set(NAMES)


def test_companions_and_staged_keep_their_keys():
    from thunder_speech_amd import _lib
    assert list(_lib.STAGED) == ["mxfp8"]
    assert sorted(_lib.COMPANIONS) == sorted(os.path.basename(p)[:-2] for p in glob.glob(os.path.join(ROOT, "include", "thunder_speech_amd", "*.h")))
    assert len(_lib.COMPANIONS) == 14 and "lora_bank" not in _lib.COMPANIONS and "lora_train" in _lib.COMPANIONS
    assert _lib.SIGNATURES is _lib.CORE.signatures and not set(NAMES) & set(_lib.SIGNATURES) and _lib.ABI_VERSION == _lib.CORE.abi_version


def test_built_library_defines_both_names():
    from thunder_speech_amd import build as b
    path = b.build(verbose=False)
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert not [n for n in NAMES if n not in defined]


def test_editing_the_queued_header_makes_the_library_stale(tmp_path, monkeypatch):
    from thunder_speech_amd import _lib, build as b
    header = _lib.QUEUED["lora_bank"].path
    assert header in b.header_deps()
    lib = tmp_path / "lib.so"
    lib.write_bytes(b"")
    monkeypatch.setattr(b, "lib_path", lambda: str(lib))
    real = glob.glob
    monkeypatch.setattr(b, "sources", lambda: [])
    monkeypatch.setattr(b.glob, "glob", lambda pat, **kw: [p for p in real(pat, **kw) if p == header])
    mtime = os.path.getmtime(header)
    os.utime(lib, (mtime + 10, mtime + 10))
    assert not b.needs_build()
    os.utime(lib, (mtime - 10, mtime - 10))
    assert b.needs_build()


# ---- bookkeeping, on the host --------------------------------------------------------------------------------------------------------------------
def _adapt(cls="Wav2Vec2", precision="bf16", **kw):
    transformers = pytest.importorskip("transformers")
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    torch.manual_seed(0)
    model = getattr(transformers, cls + "Model")(getattr(transformers, cls + "Config")(**{**CFG, **kw}))
    return model, HuggingFaceEncoderAdapt(model, precision=precision, train_precision="bf16")


def _adaptation(rank=8, targets=QV, seed=1, **kw):
    """What lora_state_dict() exports from a throw-away copy, with B random and non-zero."""
    _, enc = _adapt(**kw)
    named = enc.lora_finetuning(rank=rank, alpha=16.0, targets=targets)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in named.items():
            if n.endswith("lora_B"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    return enc.lora_state_dict()


def test_bank_keeps_the_state_dict_and_retires_graphs():
    _, enc = _adapt()
    keys, epoch = list(enc.state_dict()), getattr(enc, "_param_epoch", 0)
    enc.lora_bank(rank=8, alpha_default=16.0, targets=("v_proj", "q_proj"), capacity=3)
    assert list(enc.state_dict()) == keys and enc._param_epoch == epoch + 1
    assert not [n for n, _ in enc.named_parameters() if "bank" in n] and not list(enc.buffers())
    bank = enc._lora_bank
    assert bank.targets == QV                                                     # LORA_TARGETS' order, whatever the caller's
    assert tuple(bank.a_qkv.shape) == (2, 3, 2, 8, 128) and tuple(bank.b_qkv.shape) == (2, 3, 2, 128, 8) and bank.a_out is None
    assert bank.a_qkv.dtype == torch.bfloat16 and bank.scales.dtype == torch.float32 and tuple(bank.scales.shape) == (3,)
    assert bank.ids.dtype == torch.int32 and tuple(bank.ids.shape) == (4096,) and bool((bank.ids == -1).all())
    assert enc.lora_bank_names() == [] and enc.selected_adapters() == []
    _, enc32 = _adapt(precision="fp32")
    enc32.lora_bank(rank=16, targets=ALL, capacity=1)
    assert enc32._lora_bank.a_qkv.dtype == torch.float32 and tuple(enc32._lora_bank.a_qkv.shape) == (2, 1, 3, 16, 128)
    assert tuple(enc32._lora_bank.b_out.shape) == (2, 1, 1, 128, 16)


def test_add_remove_names_round_trip_at_fixed_addresses():
    _, enc = _adapt()
    enc.lora_bank(rank=8, alpha_default=16.0, targets=QV, capacity=3)
    bank = enc._lora_bank
    ptrs = [t.data_ptr() for t in (bank.a_qkv, bank.b_qkv, bank.scales, bank.ids)]
    sds = {n: _adaptation(seed=s) for n, s in (("de", 1), ("fr", 2), ("sw", 3))}
    assert enc.lora_bank_add("de", sds["de"]) == 0 and enc.lora_bank_add("fr", sds["fr"], alpha=4.0) == 1
    assert enc.lora_bank_names() == ["de", "fr"]
    assert bank.scales.tolist() == [2.0, 0.5, 0.0]
    for slot, name in enumerate(("de", "fr")):
        for i in range(2):
            for j, t in enumerate(QV):
                assert torch.equal(bank.a_qkv[i, slot, j], sds[name][f"lora.layers.{i}.{t}.lora_A"].to(torch.bfloat16))
                assert torch.equal(bank.b_qkv[i, slot, j], sds[name][f"lora.layers.{i}.{t}.lora_B"].to(torch.bfloat16))
    enc.select_adapters(["fr", None, "de", "fr"])
    enc.lora_bank_remove("de")
    assert enc.lora_bank_names() == ["fr"] and not bool(bank.a_qkv[:, 0].any()) and not bool(bank.b_qkv[:, 0].any()) and bank.scales[0] == 0
    assert bank.ids[:5].tolist() == [1, -1, -1, 1, -1] and enc.selected_adapters() == ["fr", None, None, "fr"]
    assert enc.lora_bank_add("sw", sds["sw"]) == 0 and enc.lora_bank_add("de", sds["de"]) == 2      # the first free slot
    assert enc.lora_bank_names() == ["sw", "fr", "de"]
    assert ptrs == [t.data_ptr() for t in (bank.a_qkv, bank.b_qkv, bank.scales, bank.ids)]


def test_select_adapters_resolves_names_and_pads_with_minus_one():
    _, enc = _adapt()
    enc.lora_bank(rank=8, targets=QV, capacity=4)
    epoch = enc._param_epoch
    for n, s in (("a", 1), ("b", 2), ("c", 3)):
        enc.lora_bank_add(n, _adaptation(seed=s))
    enc.select_adapters(["c", None, "a", "a", "b"])
    ids = enc._lora_bank.ids
    assert ids[:5].tolist() == [2, -1, 0, 0, 1] and bool((ids[5:] == -1).all())
    assert enc.selected_adapters() == ["c", None, "a", "a", "b"]
    enc.select_adapters(["b"])
    assert ids[:2].tolist() == [1, -1] and bool((ids[1:] == -1).all())
    enc.select_adapters([])
    assert bool((ids == -1).all())
    enc.select_adapters(["a"] * 4096)
    assert bool((ids == 0).all())
    assert enc._param_epoch == epoch                                               # no stamp change: nothing is re-captured
    with pytest.raises(KeyError, match="'nope'"):
        enc.select_adapters(["a", "nope"])
    assert bool((ids == 0).all())                                                  # a refused selection changes nothing
    with pytest.raises(ValueError, match="4096"):
        enc.select_adapters([None] * 4097)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_of_lora_bank_are_value_errors():
    _, enc = _adapt()
    for rank in (0, 4, 12, 128, 8.0, True):
        with pytest.raises(ValueError, match="rank"):
            enc.lora_bank(rank=rank)
    for targets in (("q_proj", "w_proj"), (), ("q_proj", "q_proj")):
        with pytest.raises(ValueError, match="targets"):
            enc.lora_bank(targets=targets)
    with pytest.raises(ValueError, match="alpha_default"):
        enc.lora_bank(alpha_default=0.0)
    for capacity in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="capacity"):
            enc.lora_bank(capacity=capacity)
    assert getattr(enc, "_lora_bank", None) is None


def test_lora_bank_refuses_by_name():
    _, enc = _adapt(precision="mxfp8")
    with pytest.raises(NotImplementedError, match="mxfp8"):
        enc.lora_bank()
    _, enc = _adapt()
    enc.lora_finetuning(rank=8)
    with pytest.raises(RuntimeError, match="carries LoRA parameters"):
        enc.lora_bank()
    _, enc = _adapt()
    enc.lora_bank()
    with pytest.raises(RuntimeError, match="already has a LoRA bank"):
        enc.lora_bank()
    with pytest.raises(RuntimeError, match="serves a LoRA bank"):
        enc.lora_finetuning(rank=8)
    assert getattr(enc, "lora", None) is None
    _, bare = _adapt()
    for call in (lambda: bare.lora_bank_add("a", {}), lambda: bare.lora_bank_remove("a"), bare.lora_bank_names, lambda: bare.select_adapters([]),
                 bare.selected_adapters):
        with pytest.raises(RuntimeError, match="no LoRA bank"):
            call()


@pytest.mark.parametrize("cls,kw", [
    ("Wav2Vec2Conformer", dict(position_embeddings_type="rotary", hidden_size=128, num_attention_heads=2, conv_depthwise_kernel_size=7)),
    ("SEW", dict(squeeze_factor=2)),
    ("Wav2Vec2", dict(adapter_attn_dim=16, do_stable_layer_norm=True, feat_extract_norm="layer")),
    ("Wav2Vec2", dict(hidden_size=144, num_attention_heads=2, num_conv_pos_embedding_groups=2)),
])
def test_refused_model_types_get_refuse_loras_own_message(cls, kw):
    from thunder_speech_amd.huggingface.train import refuse_lora
    model, enc = _adapt(cls=cls, **kw)
    with pytest.raises(NotImplementedError) as want:
        refuse_lora(model.config)
    with pytest.raises(NotImplementedError) as got:
        enc.lora_bank()
    assert str(got.value) == str(want.value) and getattr(enc, "_lora_bank", None) is None


def test_lora_bank_add_checks_keys_shapes_names_and_room():
    _, enc = _adapt()
    enc.lora_bank(rank=8, targets=QV, capacity=2)
    sd = _adaptation()
    with pytest.raises(KeyError, match="keys differ"):
        enc.lora_bank_add("a", {k: v for k, v in sd.items() if "layers.1.v_proj.lora_B" not in k})
    with pytest.raises(KeyError, match="unexpected"):
        enc.lora_bank_add("a", _adaptation(targets=ALL))
    with pytest.raises(ValueError, match=r"shape \(16, 128\)"):
        enc.lora_bank_add("a", _adaptation(rank=16))
    with pytest.raises(ValueError, match="alpha"):
        enc.lora_bank_add("a", sd, alpha=-1.0)
    with pytest.raises(ValueError, match="name"):
        enc.lora_bank_add("", sd)
    assert enc.lora_bank_names() == [] and not bool(enc._lora_bank.b_qkv.any())
    enc.lora_bank_add("a", sd)
    with pytest.raises(RuntimeError, match="already holds an adaptation named 'a'"):
        enc.lora_bank_add("a", sd)
    enc.lora_bank_add("b", sd)
    with pytest.raises(RuntimeError, match="full"):
        enc.lora_bank_add("c", sd)
    with pytest.raises(KeyError, match="'zz'"):
        enc.lora_bank_remove("zz")


def test_train_mode_with_a_bank_is_refused_before_the_gpu_check():
    _, enc = _adapt()
    enc.lora_bank()
    enc.train()
    with pytest.raises(NotImplementedError, match="LoRA bank"):
        enc(torch.zeros(1, 4000), torch.tensor([4000]))                             # CPU tensors: the refusal by name comes first


def test_a_forward_with_a_bank_refuses_by_name_before_the_gpu_check():
    _, enc = _adapt()
    enc.lora_bank()
    enc.eval()
    with pytest.raises(RuntimeError, match="4096"):
        enc(torch.zeros(4097, 400), torch.full((4097,), 400))
    enc.precision = "fp32"
    with pytest.raises(RuntimeError, match="precision='bf16'"):
        enc(torch.zeros(1, 4000), torch.tensor([4000]))


def test_predict_adapted_names_an_encoder_without_a_bank():
    from thunder_speech_amd.module import BaseCTCModule

    class Other(torch.nn.Module):
        pass
    stub = BaseCTCModule.__new__(BaseCTCModule)
    torch.nn.Module.__init__(stub)
    stub.encoder = Other()
    with pytest.raises(NotImplementedError, match="Other"):
        stub.predict_adapted(torch.zeros(1, 400), [None])
