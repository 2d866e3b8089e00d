"""Head_dim 80 fine-tuning on the CPU (the companion C header: tests/test_abi_headers_host.py): which geometries the two fused attention
nodes take, and that a head_dim 80 model in mixed precision is no longer refused before the GPU check."""
import pytest
import torch


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
