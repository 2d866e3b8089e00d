"""Head_dim 80 fine-tuning on the CPU: the companion C header include/thunder_speech_amd_mms_train.h next to the unchanged other headers, its
binding in _lib, the symbols of the built library, which geometries the two fused attention nodes take, and that a head_dim 80 model in mixed
precision is no longer refused before the GPU check."""
import ctypes
import glob
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "thunder_speech_amd_mms_train.h")
NAMES = sorted(["ts_mms_train_abi_version", "ts_mms_attention_train_fwd_workspace", "ts_mms_attention_train_fwd",
                "ts_mms_attention_train_bwd_workspace", "ts_mms_attention_train_bwd"])


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ts_[a-z0-9_]+)\s*\(", src)))


def test_companion_header_parses_and_is_version_1():
    from thunder_speech_amd import _lib
    assert _lib.MMS_TRAIN_HEADER == HEADER
    sigs, structs, defines = _lib.read_header(open(HEADER).read())
    assert defines["TS_MMS_TRAIN_ABI_VERSION"] == 1 and _lib.MMS_TRAIN_ABI_VERSION == 1 and not structs
    assert sorted(sigs) == _declared(HEADER) == NAMES


def test_its_five_names_are_declared_nowhere_else():
    from thunder_speech_amd import _lib
    others = [h for h in glob.glob(os.path.join(ROOT, "include", "*.h")) if h != HEADER]
    assert len(others) >= 5
    for h in others:
        assert not set(_declared(h)) & set(NAMES), h
    for table in (_lib.SIGNATURES, _lib.WAVLM_SIGNATURES, _lib.WAVLM_TRAIN_SIGNATURES, _lib.CONFORMER_SIGNATURES, _lib.MMS_SIGNATURES):
        assert not set(table) & set(NAMES)


def test_lib_signatures_match_the_header_exactly():
    from thunder_speech_amd import _lib
    sigs, _, _ = _lib.read_header(open(HEADER).read())
    assert _lib.MMS_TRAIN_SIGNATURES == sigs and sorted(_lib.MMS_TRAIN_SIGNATURES) == NAMES
    vp, i32, i64, u64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float
    assert sigs["ts_mms_train_abi_version"] == (ctypes.c_int, [])
    assert sigs["ts_mms_attention_train_fwd_workspace"] == (i64, [i32, i32, i32, i32])
    assert sigs["ts_mms_attention_train_bwd_workspace"] == (i64, [i32, i32, i32, i32])
    assert sigs["ts_mms_attention_train_fwd"] == (ctypes.c_int, [vp, i32, i32, i32, i32, vp, f32, u64, vp, vp, vp, vp])
    assert sigs["ts_mms_attention_train_bwd"] == (ctypes.c_int, [vp, i32, i32, i32, i32, vp, f32, u64, vp, vp, vp, vp, vp, vp, vp])


def test_built_library_defines_the_five_symbols():
    from thunder_speech_amd import _lib, build as b
    path = b.build(verbose=False)
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert set(NAMES) <= defined and set(_lib.MMS_TRAIN_SIGNATURES) <= defined


def test_which_geometries_the_fused_nodes_take():
    from thunder_speech_amd.huggingface import train as T
    for c, heads in ((1280, 16), (160, 2)):
        assert T.AttentionFused80.supported(c, heads) and not T.AttentionFused.supported(c, heads)
    for c, heads in ((1024, 16), (192, 2), (100, 3)):
        assert not T.AttentionFused80.supported(c, heads)
    # head_dim 64 stays AttentionFused's, and only that
    assert T.AttentionFused.supported(1024, 16) and T.AttentionFused.supported(128, 2) and T.AttentionFused.supported(64, 1)
    assert not T.AttentionFused.supported(192, 2) and not T.AttentionFused.supported(100, 3) and not T.AttentionFused.supported(768, 8)
    assert T.AttentionFused80.__name__ == "AttentionFused80" and T.AttentionFused80 is not T.AttentionFused
    assert T.FUSED_ATTENTION is True


def test_a_head_dim_80_model_in_mixed_precision_reaches_the_gpu_check():
    transformers = pytest.importorskip("transformers")
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    cfg = transformers.Wav2Vec2Config(hidden_size=160, num_hidden_layers=2, num_attention_heads=2, intermediate_size=320, feat_extract_norm="layer",
                                      conv_bias=True, do_stable_layer_norm=True, vocab_size=32, conv_dim=(32,) * 7,
                                      conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_stride=(5, 2, 2, 2, 2, 2, 2), num_conv_pos_embeddings=16,
                                      num_conv_pos_embedding_groups=4)
    enc = HuggingFaceEncoderAdapt(transformers.Wav2Vec2Model(cfg), train_precision="bf16")
    enc.train()
    with pytest.raises(RuntimeError) as e:                     # CPU tensors: no refusal by name comes first, the GPU check does (no CPU path)
        enc(torch.zeros(1, 4000), torch.tensor([4000]))
    assert not isinstance(e.value, NotImplementedError)
