"""GPU parity of the WavLM path (csrc/wavlm.hip through include/thunder_speech_amd/wavlm.h, then the whole encoder through the loader) against
transformers' own WavLM modules in f32 on the CPU and against a float64 restatement of the gated relative-position attention."""
import json
import os

import numpy as np
import pytest
import torch

transformers = pytest.importorskip("transformers")

pytestmark = pytest.mark.gpu

VOCAB = ["<pad>", "<s>", "</s>", "<unk>", "|"] + list("abcdefghijklmnopqrstuvwxyz'")
CFG = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, vocab_size=len(VOCAB), conv_dim=(32,) * 7,
           conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_stride=(5, 2, 2, 2, 2, 2, 2), num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4,
           pad_token_id=0)
FAMILIES = {"base": dict(feat_extract_norm="group", do_stable_layer_norm=False),
            "base-conv-bias": dict(feat_extract_norm="group", do_stable_layer_norm=False, conv_bias=True),
            "large": dict(feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True),
            "large-no-conv-bias": dict(feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=False),
            "base-adapter": dict(feat_extract_norm="group", do_stable_layer_norm=False, add_adapter=True, num_adapter_layers=1, output_hidden_size=64)}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bias_diagonals(embed, nb, md, t):
    from thunder_speech_amd import _lib
    from thunder_speech_amd.huggingface.encoder import wavlm_bucket_table
    L = _lib.lib()
    heads = embed.shape[1]
    rb = torch.full((heads, 2 * t - 1), float("nan"), device="cuda")
    table = wavlm_bucket_table(nb, md).cuda()
    assert L.ts_wavlm_rel_bias(embed.cuda().data_ptr(), table.data_ptr(), nb, md, heads, t, rb.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    return rb.cpu()


def _full_bias(rb, t):
    """[H][t][t] from the diagonals: bias[h][i][j] = rb[h][j - i + t - 1]."""
    idx = torch.arange(t)[None, :] - torch.arange(t)[:, None] + t - 1
    return rb[:, idx]


@pytest.mark.parametrize("t", [1, 7, 80, 81, 500, 1001])
def test_rel_bias_equals_compute_bias_bit_for_bit(t):
    from transformers.models.wavlm.modeling_wavlm import WavLMAttention
    torch.manual_seed(t)
    att = WavLMAttention(256, 4)                         # default 320 buckets / max distance 800
    with torch.no_grad():
        att.rel_attn_embed.weight.copy_(torch.randn(320, 4))
        want = att.compute_bias(t, t)                    # [H][t][t]
    got = _full_bias(_bias_diagonals(att.rel_attn_embed.weight.detach(), 320, 800, t), t)
    assert torch.equal(got, want)


def _reference(qkv, gx, heads, key_len, E, wg, bg, cst, nb, md):
    """float64 restatement of WavLMAttention's core: softmax(q k^T / 8 + gate rb + key mask) v; a clip without a valid key softmaxes over all keys."""
    from thunder_speech_amd.huggingface.encoder import relative_position_bucket
    b, t, c3 = qkv.shape
    c = c3 // 3
    q, k, v = [z.view(b, t, heads, 64).transpose(1, 2).double() for z in qkv.split(c, dim=-1)]
    xh = gx.double().view(b, t, heads, 64).transpose(1, 2)
    p = xh @ wg.double().T + bg.double()
    a, g = torch.sigmoid(p[..., :4].sum(-1)), torch.sigmoid(p[..., 4:].sum(-1))
    gate = a * (g * cst.double()[None, :, None] - 1.0) + 2.0                     # [b][H][t]
    rp = torch.arange(t)[None, :] - torch.arange(t)[:, None]
    rb = E.double()[relative_position_bucket(rp, nb, md)].permute(2, 0, 1)     # [H][t][t]
    s = (q @ k.transpose(-1, -2)) / 8.0 + gate[..., None] * rb[None]
    if key_len is not None:
        n = key_len.long()
        pad = (torch.arange(t)[None, :] >= n[:, None]) & (n[:, None] > 0)
        s = s.masked_fill(pad[:, None, None, :], float("-inf"))
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(b, t, c)


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("b,t,heads,lens", [(2, 1, 1, None), (2, 63, 2, [63, 1]), (1, 64, 1, None), (3, 65, 2, [65, 0, 30]),
                                            (2, 129, 3, [129, 100]), (2, 999, 2, [999, 437]), (1, 999, 1, None)])
def test_attention_matches_a_float64_restatement(precision, b, t, heads, lens):
    from thunder_speech_amd import _lib
    L = _lib.lib()
    c, nb, md = 64 * heads, 320, 800
    g = torch.Generator().manual_seed(1000 * t + 10 * heads + precision)
    qkv = torch.randn(b, t, 3 * c, generator=g)
    gx = torch.randn(b, t, c, generator=g)
    E = 2.0 * torch.randn(nb, heads, generator=g)
    wg, bg = 0.2 * torch.randn(8, 64, generator=g), 0.5 * torch.randn(8, generator=g)
    cst = 1.0 + 0.5 * torch.randn(heads, generator=g)
    if precision:                                       # the kernel reads bf16 qkv and gate input; so does the restatement
        qkv, gx = qkv.to(torch.bfloat16), gx.to(torch.bfloat16)
    key_len = torch.tensor(lens, dtype=torch.int32) if lens is not None else None
    ref = _reference(qkv.float(), gx.float(), heads, key_len, E, wg, bg, cst, nb, md)
    ref0 = _reference(qkv.float(), gx.float(), heads, key_len, torch.zeros_like(E), wg, bg, cst, nb, md)
    rb = _bias_diagonals(E, nb, md, t).cuda()
    dq, dx = qkv.cuda(), gx.cuda()
    dwg, dbg, dcst = wg.cuda(), bg.cuda(), cst.cuda()
    ctx = torch.full((b, t, c), float("nan"), dtype=qkv.dtype, device="cuda")
    n_ws = L.ts_wavlm_attention_workspace_bytes(b, t, heads, precision)
    assert n_ws == (0 if precision else b * heads * t * t * 4)
    ws = torch.empty(max(n_ws, 1), dtype=torch.uint8, device="cuda")
    kl = key_len.cuda() if key_len is not None else None
    st = L.ts_wavlm_attention_fwd(dq.data_ptr(), b, t, c, heads, kl.data_ptr() if kl is not None else None, precision, dx.data_ptr(), c,
                                  dwg.data_ptr(), dbg.data_ptr(), dcst.data_ptr(), rb.data_ptr(), ctx.data_ptr(), ws.data_ptr() if n_ws else None,
                                  _stream())
    assert st == 0
    torch.cuda.synchronize()
    got = ctx.double().cpu()
    scale = max(1.0, float(ref.abs().max()))
    if precision == 0:
        tol = 1e-5 * scale
        assert float((got - ref).abs().max()) <= tol
    else:
        tol = 0.03 * scale                               # the fused wav2vec2 kernel's bounds: bf16 probabilities and a bf16 result
        assert float((got - ref).abs().max()) <= tol
        assert float((got - ref).pow(2).mean().sqrt()) <= 0.006 * scale
    if t > 1:                                            # a kernel without the bias (or the gate) lands near ref0, not ref
        assert float((got - ref0).abs().max()) >= 10 * tol


def _random_wavlm_ctc(family, seed, layers=2, nb=32, md=40):
    torch.manual_seed(seed)
    cfg = transformers.WavLMConfig(**{**CFG, **FAMILIES[family], "num_hidden_layers": layers, "num_buckets": nb, "max_bucket_distance": md})
    model = transformers.WavLMForCTC(cfg).eval()
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if k.endswith(".bias"):
                v.copy_(0.1 * torch.randn_like(v))
            elif k.endswith("rel_attn_embed.weight"):
                v.copy_(1.5 * torch.randn_like(v))         # the bias term O(1)
            elif k.endswith("gru_rel_pos_const"):
                v.copy_(1.0 + 0.5 * torch.randn_like(v))
            elif k.endswith("gru_rel_pos_linear.weight"):
                v.copy_(0.1 * torch.randn_like(v))
    return model


def _encoder(model, precision, mask_input=False):
    from thunder_speech_amd.huggingface.compatibility import module_from_huggingface
    fe = transformers.Wav2Vec2FeatureExtractor(return_attention_mask=mask_input)
    m = module_from_huggingface(model, fe, None)
    m.encoder.precision = precision
    return m.cuda()


@pytest.mark.parametrize("family", list(FAMILIES))
def test_encoder_matches_transformers(family):
    """Small buckets (32 / 40): the exact (|d| < 8), log and clamped (|d| >= 40) branches all occur within the 75 frames."""
    model = _random_wavlm_ctc(family, seed=5)
    x = torch.randn(2, 75 * 320 + 80)
    with torch.no_grad():
        want = model.base_model(x).last_hidden_state
    assert want.shape[1] == (38 if "adapter" in family else 75)        # the adapter layer halves the encoder's 75 frames
    for precision in ("fp32", "bf16"):
        m = _encoder(model, precision)
        with torch.no_grad():
            h, out_len = m.encoder(x.cuda(), torch.tensor([x.shape[1]] * 2).cuda())
        got = h.transpose(1, 2).cpu()
        assert got.shape == want.shape and out_len.tolist() == [want.shape[1]] * 2
        if precision == "fp32":
            np.testing.assert_allclose(got.numpy(), want.numpy(), atol=5e-4, rtol=1e-4)
        else:
            assert float((got - want).abs().max()) <= 0.1 and float((got - want).pow(2).mean().sqrt()) <= 0.01


@pytest.mark.parametrize("family", ["base", "large"])
def test_encoder_with_ragged_lengths_matches_transformers_on_valid_frames(family):
    model = _random_wavlm_ctc(family, seed=7)
    n = 75 * 320 + 80
    lengths = torch.tensor([n, 41 * 320 + 80])
    x = torch.randn(2, n)
    x[1, lengths[1]:] = 0
    mask = (torch.arange(n)[None, :] < lengths[:, None]).long()
    with torch.no_grad():
        want = model.base_model(x, attention_mask=mask).last_hidden_state
    for precision in ("fp32", "bf16"):
        m = _encoder(model, precision, mask_input=True)
        assert m.encoder.mask_input
        with torch.no_grad():
            h, out_len = m.encoder(x.cuda(), lengths.cuda())
        got = h.transpose(1, 2).cpu()
        assert out_len.tolist() == [75, 41]
        for i, n_i in enumerate(out_len.tolist()):
            g, w = got[i, :n_i], want[i, :n_i]
            if precision == "fp32":
                np.testing.assert_allclose(g.numpy(), w.numpy(), atol=5e-4, rtol=1e-4)
            else:
                assert float((g - w).abs().max()) <= 0.1 and float((g - w).pow(2).mean().sqrt()) <= 0.01


def test_one_layer_encoder_beyond_max_distance_at_the_default_buckets():
    """320 / 800 buckets and t = 802 > 800 frames: the clamped bucket at the published geometry."""
    model = _random_wavlm_ctc("large", seed=9, layers=1, nb=320, md=800)
    x = torch.randn(1, 802 * 320 + 80)
    with torch.no_grad():
        want = model.base_model(x).last_hidden_state
    assert want.shape[1] == 802
    for precision in ("fp32", "bf16"):
        m = _encoder(model, precision)
        with torch.no_grad():
            h, _ = m.encoder(x.cuda(), torch.tensor([x.shape[1]]).cuda())
        got = h.transpose(1, 2).cpu()
        if precision == "fp32":
            np.testing.assert_allclose(got.numpy(), want.numpy(), atol=5e-4, rtol=1e-4)
        else:
            assert float((got - want).abs().max()) <= 0.1 and float((got - want).pow(2).mean().sqrt()) <= 0.01


def _fit_margin_head(model, xn, margin=8.0):
    """lm_head fitted (ridge least squares on transformers' own hidden states) so that every frame's top-1 leads its top-2 by ~`margin`:
    a pattern of letters and blanks, so the greedy strings are not empty and no bf16 deviation can flip a frame."""
    with torch.no_grad():
        h = model.base_model(xn).last_hidden_state                     # [B][T][C]
    b, t, c = h.shape
    labels = torch.zeros(b, t, dtype=torch.long)
    for i in range(b):
        for f in range(t):
            labels[i, f] = 0 if (f // 3) % 2 else 5 + (3 * i + f // 6) % 26
    target = torch.full((b * t, len(VOCAB)), -margin / 2)
    target[torch.arange(b * t), labels.reshape(-1)] = margin / 2
    hf = torch.cat([h.reshape(b * t, c), torch.ones(b * t, 1)], 1).double()
    # the ridge term keeps the head's norm (and with it the bf16 deviation of the logits) down; it costs ~40 % of the margin
    w = torch.linalg.solve(hf.T @ hf + torch.eye(c + 1, dtype=torch.float64), hf.T @ target.double())
    with torch.no_grad():
        model.lm_head.weight.copy_(w[:c].T.float())
        model.lm_head.bias.copy_(w[c].float())


def _save_checkpoint(model, d):
    model.save_pretrained(d)
    with open(os.path.join(d, "vocab.json"), "w") as f:
        json.dump({tok: i for i, tok in enumerate(VOCAB)}, f)
    transformers.Wav2Vec2CTCTokenizer(os.path.join(d, "vocab.json")).save_pretrained(d)
    transformers.Wav2Vec2FeatureExtractor(return_attention_mask=False).save_pretrained(d)


def test_checkpoint_directory_loads_and_predicts(tmp_path):
    """Two save_pretrained directories of one WavLMForCTC: with its randomly initialised head (logits against transformers' within the loader
    test's bf16 bound) and with a margin-fitted head (the head's norm amplifies the bf16 deviation of the hidden states past that bound, but every
    frame's decision is far from a tie: predict() must give the greedy strings of transformers' logits, eagerly, captured and replayed)."""
    from thunder_speech_amd.huggingface.compatibility import load_huggingface_checkpoint
    from thunder_speech_amd.module import greedy_decode
    model = _random_wavlm_ctc("base", seed=11)
    g = torch.Generator().manual_seed(12)
    x = 0.1 * torch.randn(2, 30 * 320 + 80, generator=g)
    xn = (x - x.mean(dim=1, keepdim=True)) / torch.sqrt(x.var(dim=1, keepdim=True) + 1e-7)     # Wav2Vec2Preprocess, mask_input=False
    lengths = torch.tensor([x.shape[1]] * 2).cuda()

    _save_checkpoint(model, str(tmp_path / "random_head"))
    with torch.no_grad():
        ref = model(xn).logits.transpose(1, 2)                          # [B][V][T]
    m = load_huggingface_checkpoint(str(tmp_path / "random_head"))
    assert m.encoder.original_encoder.config.model_type == "wavlm" and m.encoder.precision == "bf16"
    m = m.cuda()
    with torch.no_grad():
        logits, out_len = m(x.cuda(), lengths)
    assert logits.shape == ref.shape and out_len.tolist() == [ref.shape[2]] * 2
    assert float((logits.float().cpu() - ref).abs().max()) <= 0.02 * max(1.0, float(ref.abs().max()))

    _fit_margin_head(model, xn)
    _save_checkpoint(model, str(tmp_path / "margin_head"))
    with torch.no_grad():
        ref = model(xn).logits.transpose(1, 2)
    top2 = ref.topk(2, dim=1).values
    scale = max(1.0, float(ref.abs().max()))
    assert float((top2[:, 0] - top2[:, 1]).min()) > 0.5 * scale         # the fitted head leaves every frame far from a tie
    m = load_huggingface_checkpoint(str(tmp_path / "margin_head")).cuda()
    m.graph_inference = True
    with torch.no_grad():
        logits, _ = m(x.cuda(), lengths)
        texts = [m.predict(x.cuda()) for _ in range(3)]                 # eager, then captured, then replayed
    assert torch.equal(logits.float().argmax(1).cpu(), ref.argmax(1))
    _, collapsed, counts = greedy_decode(ref.cuda())
    want = m.text_transform.decode_collapsed(collapsed, counts)
    assert all(len(s) > 0 for s in want)
    assert texts[0] == want and texts[1] == texts[0] and texts[2] == texts[0]
