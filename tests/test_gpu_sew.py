"""GPU parity of the SEW path: the two launches of csrc/sew.hip (through include/thunder_speech_amd/sew.h) against float64 on the CPU, element by
element, then the whole encoder against transformers' own SEWModel in f32 on the CPU, bare and through the loader.  Every output starts as NaN,
every workspace as 0xFF bytes, every return code is asserted.  Bounds of the kernel tests:
  precision 0, and precision 1 at a width without a matrix-core kernel (f32 operands)    1e-5 x max |reference| (the f32 row kernels' figure)
  precision 1 on the matrix cores                                                          max 0.03, rms 0.006 of max |reference|, the reference reading
                                                                                           the same bf16-rounded x and w for the conv and the f32 x for
                                                                                           the pool (tests/test_gpu_posconv_stack_kernels.py's bound)"""
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

transformers = pytest.importorskip("transformers")

pytestmark = pytest.mark.gpu

NAN = float("nan")
BF = torch.bfloat16
B = 2
GEOMETRIES = {"c128_g4": (128, 4), "c192_g8": (192, 8), "c256_g4": (256, 4)}       # 32 channels per group; 24 (the padded path); 64 (f32 in both precisions)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _api():
    from thunder_speech_amd import _lib
    return _lib, _lib.lib()


def _nan(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device="cuda")


def _ws(nbytes):
    assert nbytes > 0
    return torch.full((int(nbytes),), 0xFF, dtype=torch.uint8, device="cuda")


# ---------------------------------------------------------------------------------------------------------------------
# 1. ts_sew_squeeze_fwd
# ---------------------------------------------------------------------------------------------------------------------
def _squeeze_ref(x_conv, x_pool, w, bias, groups, s):
    """float64: mean_{i < s} x_pool[s r + i] + gelu(conv_stride_s(x_conv) + bias) for r < T // s; x [B][T][C], w [C][C / groups][k]."""
    t, k = x_pool.shape[1], w.shape[2]
    t2 = t // s
    conv = F.conv1d(x_conv.transpose(1, 2), w, bias, stride=s, padding=k // 2, groups=groups)[..., :t2]
    pool = F.avg_pool1d(x_pool.transpose(1, 2), s, s)[..., :t2]
    assert conv.shape[-1] == t2 == pool.shape[-1]
    return (pool + F.gelu(conv)).transpose(1, 2)


@functools.lru_cache(maxsize=None)
def _squeeze_case(geometry, k, s, t, zero_tail=False):
    """(x, w, bias, float64 reference of the f32 operands, float64 reference of the bf16-rounded conv operands); computed once per shape."""
    c, groups = GEOMETRIES[geometry]
    cg = c // groups
    g = torch.Generator().manual_seed(100000 * c + 1000 * k + 10 * t + s)
    x = torch.randn(B, t, c, generator=g) + 0.25 * torch.arange(B, dtype=torch.float32)[:, None, None]       # the clips hold different data
    if zero_tail:
        x[1, 2 * t // 3:] = 0.0                                                  # a masked batch: rows >= len are zero (ts_w2v_mask_rows)
    w = torch.randn(c, cg, k, generator=g) * (cg * k) ** -0.5
    bias = 0.3 * torch.randn(c, generator=g)
    ref32 = _squeeze_ref(x.double(), x.double(), w.double(), bias.double(), groups, s)
    ref16 = _squeeze_ref(x.to(BF).double(), x.double(), w.to(BF).double(), bias.double(), groups, s)
    return x, w, bias, ref32, ref16


def _squeeze_call(x, w, bias, groups, s, precision):
    """-> (status, y) of one ts_sew_squeeze_fwd call; the taps packed the way the plan packs them."""
    from thunder_speech_amd.huggingface.sew import pack_squeeze_taps, squeeze_on_matrix_cores
    _lib, L = _api()
    b, t, c = x.shape
    k = w.shape[2]
    cg = c // groups
    mfma = precision == 1 and cg in (24, 32)
    taps = pack_squeeze_taps(w.cuda(), groups, mfma)
    xs, bs = x.cuda(), bias.cuda()
    y = _nan(b, t // s, c)
    ws = _ws(L.ts_sew_squeeze_workspace_bytes(b, t, c, k, s, precision))
    st = L.ts_sew_squeeze_fwd(xs.data_ptr(), b, t, c, taps.data_ptr(), bs.data_ptr(), k, groups, s, precision, y.data_ptr(), ws.data_ptr(), _stream())
    torch.cuda.synchronize()
    if mfma and not squeeze_on_matrix_cores(cg, k, s):
        # (127 s + k) window rows x 144 bytes over 64 KiB of LDS (s = 3 with 128 taps): refused before any launch, the plan takes the f32 path
        assert st == _lib.TS_EUNSUPPORTED and bool(torch.isnan(y).all())
        return st, None
    assert st == 0
    return st, y


def _assert_squeeze(y, ref, mfma, what):
    got = y.double().cpu()
    assert got.shape == ref.shape
    assert not bool(torch.isnan(got).any()), f"{what}: unwritten (NaN) elements"
    scale = float(ref.abs().max())
    mx, rms = float((got - ref).abs().max()), float((got - ref).pow(2).mean().sqrt())
    print(f"{what}: max {mx:.3e} rms {rms:.3e} of scale {scale:.3e}")
    if mfma:
        assert mx <= 0.03 * scale and rms <= 0.006 * scale, f"{what}: max {mx:.3e} rms {rms:.3e} against scale {scale:.3e}"
    else:
        assert mx <= 1e-5 * scale, f"{what}: max error {mx:.3e} > 1e-5 x {scale:.3e}"


def _frames(s):
    """a single output frame; a ragged tail; t % s != 0 behind more than one 128-frame tile at s = 2; the same behind s x 128 frames for every s"""
    return sorted({s, 7, 261, 2 * 128 + 2 * s + 1, s * 128 + 2 * s + 1})


@pytest.mark.parametrize("s", [2, 3])
@pytest.mark.parametrize("k", [15, 16, 128])
@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_squeeze_matches_float64_in_both_precisions(geometry, k, s):
    c, groups = GEOMETRIES[geometry]
    for t in _frames(s):
        x, w, bias, ref32, ref16 = _squeeze_case(geometry, k, s, t)
        for precision in (0, 1):
            mfma = precision == 1 and c // groups in (24, 32)
            st, y = _squeeze_call(x, w, bias, groups, s, precision)
            if y is not None:
                _assert_squeeze(y, ref16 if mfma else ref32, mfma, f"squeeze {geometry} k={k} s={s} t={t} precision={precision}")


@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_squeeze_with_stride_one(geometry):
    """s = 1: the pool is x itself and the launch is wav2vec2's positional embedding."""
    c, groups = GEOMETRIES[geometry]
    for k, t in [(16, 261), (15, 1)]:
        x, w, bias, ref32, ref16 = _squeeze_case(geometry, k, 1, t)
        for precision in (0, 1):
            mfma = precision == 1 and c // groups in (24, 32)
            st, y = _squeeze_call(x, w, bias, groups, 1, precision)
            _assert_squeeze(y, ref16 if mfma else ref32, mfma, f"squeeze {geometry} k={k} s=1 t={t} precision={precision}")


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_two_squeeze_calls_give_equal_bits(geometry, precision):
    c, groups = GEOMETRIES[geometry]
    x, w, bias, _, _ = _squeeze_case(geometry, 128, 2, 261)
    (_, y0), (_, y1) = _squeeze_call(x, w, bias, groups, 2, precision), _squeeze_call(x, w, bias, groups, 2, precision)
    assert not bool(torch.isnan(y0).any()) and torch.equal(y0, y1)


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_squeeze_of_a_masked_batch_equals_the_restatement_on_the_masked_input(geometry, precision):
    """Clip 1's rows from two thirds on are zero, as ts_w2v_mask_rows leaves them: the taps that reach into them and the pool over them read zeros."""
    c, groups = GEOMETRIES[geometry]
    for s, k in [(2, 16), (3, 15)]:
        x, w, bias, ref32, ref16 = _squeeze_case(geometry, k, s, 261, True)
        mfma = precision == 1 and c // groups in (24, 32)
        _, y = _squeeze_call(x, w, bias, groups, s, precision)
        _assert_squeeze(y, ref16 if mfma else ref32, mfma, f"masked squeeze {geometry} k={k} s={s} precision={precision}")


# ---------------------------------------------------------------------------------------------------------------------
# 2. ts_sew_unsqueeze_rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,rest", [(2, 1), (3, 1), (3, 2)])                      # t - s t2 in {1, s - 1}
def test_unsqueeze_rows_is_an_exact_copy_with_a_zero_tail(s, rest):
    _lib, L = _api()
    c, t2 = 128, 87
    t = s * t2 + rest
    g = torch.Generator().manual_seed(s + rest)
    src = torch.randn(B, t2, s * c, generator=g)
    want = torch.cat([src.reshape(B, s * t2, c), torch.zeros(B, rest, c)], 1)
    ds = src.cuda()
    dst = _nan(B, t, c)
    assert L.ts_sew_unsqueeze_rows(ds.data_ptr(), B, t2, t, c, s, dst.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), want)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the encoder against transformers
# ---------------------------------------------------------------------------------------------------------------------
VOCAB = ["<pad>", "<s>", "</s>", "<unk>", "|"] + list("abcdefghijklmnopqrstuvwxyz'")
CFG = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, vocab_size=len(VOCAB), conv_dim=(32, 32, 32, 32, 64),
           conv_kernel=(10, 3, 1, 3, 1), conv_stride=(5, 2, 1, 2, 1), num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, squeeze_factor=2,
           layer_norm_eps=1e-3, pad_token_id=0)
VARIANTS = {"group_projection": dict(feat_extract_norm="group"),
            "layer_bias_no_projection": dict(feat_extract_norm="layer", conv_bias=True, conv_dim=(32, 32, 32, 32, 128)),
            "squeeze3_taps15": dict(feat_extract_norm="group", squeeze_factor=3, num_conv_pos_embeddings=15)}
N_ODD, N_EVEN = 4000, 4020                                                         # 199 and 200 frames behind the five conv layers (total stride 20)
N_LOADER = 630                                                                     # 30 frames: two clips give fewer rows than the head has columns, so the margin head interpolates


def _random_sew_ctc(variant, seed, **kw):
    """layer_norm_eps 1e-3, a random weight-normed positional conv (g and v), an upsampling projection of unit gain, biases 0.1 randn."""
    torch.manual_seed(seed)
    model = transformers.SEWForCTC(transformers.SEWConfig(**{**CFG, **VARIANTS[variant], **kw})).eval()
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if "pos_conv_embed" in k and not k.endswith(".bias"):
                v.copy_(0.5 + torch.rand_like(v) if v.shape[0] == 1 and v.shape[1] == 1 else 0.3 * torch.randn_like(v))
            elif k.endswith("upsample.projection.weight"):
                v.copy_(torch.randn_like(v) * v.shape[1] ** -0.5)       # pre-activations of order 1: the output is not a sliver around gelu(0)
            elif k.endswith(".bias"):
                v.copy_(0.1 * torch.randn_like(v))
    return model


def _encoder(model, precision, mask_input=False):
    from thunder_speech_amd.huggingface.compatibility import module_from_huggingface
    fe = transformers.Wav2Vec2FeatureExtractor(return_attention_mask=mask_input)
    m = module_from_huggingface(model, fe, None)
    m.encoder.precision = precision
    return m.cuda()


# bf16 mode: SEW's output is the upsampler's GELU, not a LayerNorm row, so the absolute 0.1 / 0.01 of tests/test_gpu_wavlm.py does not transfer: the
# bound is relative, max error against max |reference| and rms error against rms(reference).  Measured once against transformers on the cases of
# this file (three variants x 199 and 200 frames, and the masked batch clip by clip): max / max |ref| 0.0051 .. 0.0083, rms / rms(ref) 0.0044 .. 0.0058,
# the largest of both with the layer-norm extractor without projection.  The bounds give those maxima the headroom ratio of
# tests/test_gpu_conformer.py (measured 0.0111 -> bound 0.014, x 1.26)
BF16_MAX_REL = 0.0105
BF16_RMS_REL = 0.0073


def _close(got, want, precision, what=""):
    if precision == "fp32":
        np.testing.assert_allclose(got.numpy(), want.numpy(), atol=5e-4, rtol=1e-4)
        return
    mx = float((got - want).abs().max()) / float(want.abs().max())
    rms = float((got - want).pow(2).mean().sqrt()) / float(want.pow(2).mean().sqrt())
    print(f"bf16 {what}: max / max|ref| {mx:.4f}, rms / rms(ref) {rms:.4f}")
    assert mx <= BF16_MAX_REL and rms <= BF16_RMS_REL, (mx, rms)


def _run(model, x, lengths, precision, mask_input=False):
    m = _encoder(model, precision, mask_input)
    with torch.no_grad():
        h, out_len = m.encoder(x.cuda(), lengths.cuda())
    return h.transpose(1, 2).cpu(), out_len.cpu()


@pytest.mark.parametrize("n", [N_ODD, N_EVEN])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_encoder_matches_transformers(variant, n):
    model = _random_sew_ctc(variant, seed=5)
    x = torch.randn(2, n)
    with torch.no_grad():
        want = model.base_model(x).last_hidden_state
    t = 199 if n == N_ODD else 200
    s = model.config.squeeze_factor
    assert want.shape == (2, t, 128)
    if t % s:
        assert not bool(want[:, s * (t // s):].any())                  # transformers pads the upsampled rows with zeros up to T
    for precision in ("fp32", "bf16"):
        got, out_len = _run(model, x, torch.tensor([n] * 2), precision)
        assert got.shape == want.shape and out_len.tolist() == [t, t]
        assert torch.equal(got[:, s * (t // s):], want[:, s * (t // s):])
        _close(got, want, precision, f"{variant} t={t}")


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_encoder_with_ragged_lengths_matches_transformers_on_valid_frames(variant):
    model = _random_sew_ctc(variant, seed=7)
    lengths = torch.tensor([N_ODD, 2 * N_ODD // 3])
    x = torch.randn(2, N_ODD)
    x[1, lengths[1]:] = 0
    mask = (torch.arange(N_ODD)[None, :] < lengths[:, None]).long()
    with torch.no_grad():
        want = model.base_model(x, attention_mask=mask).last_hidden_state
        unmasked = model.base_model(x).last_hidden_state
    want_len = model.base_model._get_feat_extract_output_lengths(lengths)
    assert float((unmasked[1, :int(want_len[1])] - want[1, :int(want_len[1])]).abs().max()) >= 10 * 5e-4        # the mask is visible in clip 1
    for precision in ("fp32", "bf16"):
        got, out_len = _run(model, x, lengths, precision, mask_input=True)
        assert torch.equal(out_len, want_len)
        for i, n_i in enumerate(out_len.tolist()):
            _close(got[i, :n_i], want[i, :n_i], precision, f"{variant} masked clip {i}")


def test_bf16_mode_runs_the_squeeze_on_the_matrix_cores_and_fp32_mode_does_not():
    model = _random_sew_ctc("group_projection", seed=5)
    for precision, want in (("bf16", True), ("fp32", False)):
        plan = _encoder(model, precision).encoder._plan(torch.device("cuda"))
        assert type(plan).__name__ == "SEWPlan" and plan.sq_mfma is want and plan.sq_prec == int(want)
        assert plan.sq_w.dtype == (BF if want else torch.float32) and plan.sq_w.shape == (16, 4, 32, 32)


def test_an_input_shorter_than_the_squeeze_factor_raises():
    model = _random_sew_ctc("squeeze3_taps15", seed=5)
    m = _encoder(model, "fp32")
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="input too short"):
            m.encoder(torch.randn(1, 50).cuda(), torch.tensor([50]).cuda())        # 2 frames, squeeze_factor 3


def test_graph_replay_equals_eager_bit_for_bit():
    model = _random_sew_ctc("group_projection", seed=10)
    x = torch.randn(2, N_ODD).cuda()
    lengths = torch.tensor([N_ODD, 2 * N_ODD // 3]).cuda()
    enc = _encoder(model, "bf16", mask_input=True).encoder
    with torch.no_grad():
        eager, _ = enc(x, lengths)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            enc(x, lengths)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out, _ = enc(x, lengths)
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(out, eager)


# ---- a saved checkpoint through the loader ---------------------------------------------------------------------------------------------
def _fit_margin_head(model, xn, margin=8.0):
    """lm_head fitted (ridge least squares on transformers' own hidden states) so that every frame's top-1 leads its top-2 by ~`margin`, the way
    tests/test_gpu_conformer.py builds its head; the ridge term is 0.1 (there 1): SEW's hidden states are GELU outputs of rms ~0.6, not LayerNorm rows,
    and with 1 the fit keeps too little of the margin.  The clips have an even frame count: a zero row behind the upsampled ones would carry the same
    features in both clips and could not take a label of its own."""
    with torch.no_grad():
        h = model.base_model(xn).last_hidden_state
    b, t, c = h.shape
    labels = torch.zeros(b, t, dtype=torch.long)
    for i in range(b):
        for f in range(t):
            labels[i, f] = 0 if (f // 3) % 2 else 5 + (3 * i + f // 6) % 26
    target = torch.full((b * t, len(VOCAB)), -margin / 2)
    target[torch.arange(b * t), labels.reshape(-1)] = margin / 2
    hf = torch.cat([h.reshape(b * t, c), torch.ones(b * t, 1)], 1).double()
    w = torch.linalg.solve(hf.T @ hf + 0.1 * torch.eye(c + 1, dtype=torch.float64), hf.T @ target.double())
    with torch.no_grad():
        model.lm_head.weight.copy_(w[:c].T.float())
        model.lm_head.bias.copy_(w[c].float())


def _save_checkpoint(model, d):
    model.save_pretrained(d)
    with open(os.path.join(d, "vocab.json"), "w") as f:
        json.dump({tok: i for i, tok in enumerate(VOCAB)}, f)
    transformers.Wav2Vec2CTCTokenizer(os.path.join(d, "vocab.json")).save_pretrained(d)
    transformers.Wav2Vec2FeatureExtractor(return_attention_mask=True).save_pretrained(d)


def test_checkpoint_directory_loads_and_predicts(tmp_path):
    from thunder_speech_amd.huggingface.compatibility import load_huggingface_checkpoint
    from thunder_speech_amd.module import greedy_decode
    model = _random_sew_ctc("group_projection", seed=11)
    g = torch.Generator().manual_seed(12)
    x = 0.1 * torch.randn(2, N_LOADER, generator=g)
    n = x.shape[1]
    xn = (x - x.mean(dim=1, keepdim=True)) / torch.sqrt(x.var(dim=1, keepdim=True, unbiased=False) + 1e-7)
    lengths = torch.tensor([n] * 2).cuda()
    am = torch.ones(2, n, dtype=torch.long)

    _save_checkpoint(model, str(tmp_path / "random_head"))
    with torch.no_grad():
        ref = model(xn, attention_mask=am).logits.transpose(1, 2)
    m = load_huggingface_checkpoint(str(tmp_path / "random_head"))
    assert m.encoder.original_encoder.config.model_type == "sew" and m.encoder.precision == "bf16" and m.encoder.mask_input
    assert m.encoder_final_dimension == 128
    m = m.cuda()
    with torch.no_grad():
        logits, out_len = m(x.cuda(), lengths)
    assert logits.shape == ref.shape and out_len.tolist() == [ref.shape[2]] * 2
    assert float((logits.float().cpu() - ref).abs().max()) <= 0.02 * max(1.0, float(ref.abs().max()))

    _fit_margin_head(model, xn)
    _save_checkpoint(model, str(tmp_path / "margin_head"))
    with torch.no_grad():
        ref = model(xn, attention_mask=am).logits.transpose(1, 2)
    top2 = ref.topk(2, dim=1).values
    scale = max(1.0, float(ref.abs().max()))
    assert float((top2[:, 0] - top2[:, 1]).min()) > 0.5 * scale
    m = load_huggingface_checkpoint(str(tmp_path / "margin_head")).cuda()
    m.graph_inference = True
    xc = x.cuda()                                                       # one address: predict()'s zero-copy graph is keyed by it
    with torch.no_grad():
        logits, _ = m(xc, lengths)
        texts = [m.predict(xc) for _ in range(3)]                       # eager, then captured, then replayed
    graphs = m.__dict__.get("_infer_graphs")
    assert graphs is not None and graphs[1].count() + graphs[2].count() >= 1      # predict() did go through a captured graph
    assert torch.equal(logits.float().argmax(1).cpu(), ref.argmax(1))
    _, collapsed, counts = greedy_decode(ref.cuda())
    want = m.text_transform.decode_collapsed(collapsed, counts)
    assert all(len(s) > 0 for s in want)
    assert texts[0] == want and texts[1] == texts[0] and texts[2] == texts[0]
