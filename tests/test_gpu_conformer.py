"""GPU parity of the wav2vec2-conformer path (csrc/conformer.hip through include/thunder_speech_amd/conformer.h, then the whole encoder through
the loader) against float64 restatements of the kernels and against transformers' own Wav2Vec2Conformer modules in f32 on the CPU."""
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
           position_embeddings_type="rotary", conv_depthwise_kernel_size=31, layer_norm_eps=1e-3, pad_token_id=0)
FAMILIES = {"group": dict(feat_extract_norm="group"), "layer": dict(feat_extract_norm="layer", conv_bias=True)}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _act(x, act):
    return torch.nn.functional.gelu(x) if act == 1 else torch.nn.functional.silu(x)


# ---- kernels against float64 -----------------------------------------------------------------------------------------------------------
def _glu_dwconv_ref(u, w, scale, shift, act):
    """u [B][t][2c], w [c][k] -> act(scale dwconv(GLU(u)) + shift) [B][t][c], float64."""
    c, k = w.shape
    g = u[..., :c] * torch.sigmoid(u[..., c:])
    d = torch.nn.functional.conv1d(g.transpose(1, 2), w[:, None, :], padding=(k - 1) // 2, groups=c)
    return _act(scale[None, :, None] * d + shift[None, :, None], act).transpose(1, 2)


@pytest.mark.parametrize("act", [1, 2])
@pytest.mark.parametrize("precision", [0, 1])
# k = 3, 5, 9, 31 reach the KT = 3, 7, 15, 31 templates (zero taps around the real ones); k = 33 and 63 the tap loop of KT = 63
@pytest.mark.parametrize("b,t,c,k", [(3, 999, 1024, 31), (2, 10, 128, 31), (1, 1, 128, 31), (2, 77, 256, 3), (2, 30, 128, 5), (2, 20, 128, 9),
                                     (2, 50, 128, 33), (1, 40, 64, 63)])
def test_glu_dwconv_matches_a_float64_restatement(b, t, c, k, precision, act):
    from thunder_speech_amd import _lib
    g = torch.Generator().manual_seed(t + c + k + 10 * precision + act)
    # a different offset per clip: a halo that read across clips would land far from the restatement
    u = torch.randn(b, t, 2 * c, generator=g) + torch.arange(b, dtype=torch.float32)[:, None, None]
    w = 0.2 * torch.randn(c, k, generator=g)
    scale, shift = 1.0 + 0.2 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
    if precision:
        u = u.to(torch.bfloat16)                           # the restatement reads the same bf16 values
    ref = _glu_dwconv_ref(u.double(), w.double(), scale.double(), shift.double(), act)
    y = torch.full((b, t, c), float("nan"), dtype=u.dtype, device="cuda")
    du, dw, ds, dh = u.cuda(), w.t().contiguous().cuda(), scale.cuda(), shift.cuda()
    st = _lib.lib().ts_conformer_glu_dwconv_fwd(du.data_ptr(), b, t, c, dw.data_ptr(), k, ds.data_ptr(), dh.data_ptr(), act, precision, y.data_ptr(),
                                                _stream())
    assert st == 0
    torch.cuda.synchronize()
    got = y.double().cpu()
    scale_out = float(ref.abs().max())
    err = float((got - ref).abs().max())
    assert err <= (1e-5 if precision == 0 else 0.01) * scale_out, (err, scale_out)


def test_glu_dwconv_refuses_what_it_does_not_take():
    from thunder_speech_amd import _lib
    L = _lib.lib()
    u = torch.zeros(1, 8, 256, device="cuda")
    w, s = torch.zeros(64, 128, device="cuda"), torch.zeros(128, device="cuda")
    y = torch.zeros(1, 8, 128, device="cuda")
    call = lambda k, act=2, c=128: L.ts_conformer_glu_dwconv_fwd(u.data_ptr(), 1, 8, c, w.data_ptr(), k, s.data_ptr(), s.data_ptr(), act, 0,
                                                                 y.data_ptr(), _stream())
    assert call(31) == 0 and call(63) == 0
    assert call(32) == _lib.TS_EUNSUPPORTED and call(65) == _lib.TS_EUNSUPPORTED and call(31, act=0) == _lib.TS_EUNSUPPORTED
    assert call(31, c=100) == _lib.TS_EUNSUPPORTED
    torch.cuda.synchronize()


def _rotary_ref(y, cos, sin):
    """y [rows][c] float64, cos / sin [rows][32] -> y cos + rotate_half(y) sin per head of 64."""
    rows, c = y.shape
    yh = y.view(rows, c // 64, 64)
    rot = torch.cat([-yh[..., 32:], yh[..., :32]], -1)
    cs, sn = torch.cat([cos, cos], -1)[:, None, :], torch.cat([sin, sin], -1)[:, None, :]
    return (yh * cs + rot * sn).reshape(rows, c)


@pytest.mark.parametrize("precision", [0, 1])
# c = 64 heads: 128 / 64 (NV = 1), 384 (NV = 2), 1024 (NV = 4), 1280 (NV = 8), 2560 (NV = 16)
@pytest.mark.parametrize("b,t,heads", [(3, 75, 2), (2, 999, 16), (2, 7, 1), (2, 5, 20), (2, 9, 6), (2, 4, 40)])
def test_layernorm_rotary_matches_a_float64_restatement(b, t, heads, precision):
    from thunder_speech_amd import _lib
    from thunder_speech_amd.huggingface.conformer import rotary_table
    c = 64 * heads
    g = torch.Generator().manual_seed(b * t + heads + precision)
    x = 2.0 * torch.randn(b, t, c, generator=g) + 0.5
    w, bb = 1.0 + 0.3 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g)
    inv_freq = 1.0 / (10000 ** (torch.arange(0, 64, 2, dtype=torch.int64).float() / 64))
    table = rotary_table(inv_freq, 1000)
    xd = x.double()
    y_ref = torch.nn.functional.layer_norm(xd, (c,), w.double(), bb.double(), eps=1e-5).reshape(b * t, c)
    pos = torch.arange(b * t) % t                                    # the frame within the padded batch
    r_ref = _rotary_ref(y_ref, table[0, pos].double(), table[1, pos].double())
    dt = torch.bfloat16 if precision else torch.float32
    y, yr = torch.full((b, t, c), float("nan"), dtype=dt, device="cuda"), torch.full((b, t, c), float("nan"), dtype=dt, device="cuda")
    dx, dw, db, dtab = x.cuda(), w.cuda(), bb.cuda(), table.cuda()
    L = _lib.lib()
    call = lambda t_table: L.ts_conformer_layernorm_rotary_fwd(dx.data_ptr(), dw.data_ptr(), db.data_ptr(), 1e-5, b, t, c, heads, dtab.data_ptr(),
                                                               t_table, precision, y.data_ptr(), yr.data_ptr(), _stream())
    assert call(t - 1) == _lib.TS_EINVAL                              # a table shorter than t is refused
    assert call(1000) == 0
    torch.cuda.synchronize()
    tol = 1e-5 if precision == 0 else 0.01
    for got, ref in ((y, y_ref), (yr, r_ref)):
        got = got.double().cpu().reshape(b * t, c)
        assert float((got - ref).abs().max()) <= tol * float(ref.abs().max())
    if t > 1:                                                         # the rotation is visible: rot(y) is not y
        assert float((yr.double().cpu() - y.double().cpu()).abs().max()) > 0.1


def _pack(w):
    from thunder_speech_amd import _lib
    out = torch.empty_like(w)
    assert _lib.lib().ts_gemm_nt_pack_w(w.data_ptr(), w.shape[1], w.shape[0], w.shape[1], out.data_ptr(), _stream()) == 0
    return out


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("precision,packed", [(0, False), (1, False), (1, True)])      # packed fragments: bf16 only
def test_linear_slices_and_silu_match_a_float64_restatement(precision, act, packed):
    """q|k (n = 2c, rotated input) and v (n = c) into their column slices of one [rows][3c] buffer: the columns next to a slice keep their
    sentinel; then the FFN shape with the activation in the epilogue and a product accumulated into the residual stream in place."""
    from thunder_speech_amd import _lib
    L = _lib.lib()
    rows, c, ff = 300, 128, 512
    g = torch.Generator().manual_seed(100 * precision + 10 * act + packed)
    dt = torch.bfloat16 if precision else torch.float32
    x, xr = torch.randn(rows, c, generator=g).to(dt), torch.randn(rows, c, generator=g).to(dt)
    wqk, wv = (0.1 * torch.randn(2 * c, c, generator=g)).to(dt), (0.1 * torch.randn(c, c, generator=g)).to(dt)
    bqk, bv = 0.1 * torch.randn(2 * c, generator=g), 0.1 * torch.randn(c, generator=g)
    d = lambda z: z.cuda()
    dx, dxr, dwqk, dwv, dbqk, dbv = map(d, (x, xr, wqk, wv, bqk, bv))
    frag = (lambda w: _pack(w).data_ptr()) if packed else (lambda w: None)
    sentinel = 7.0
    qkv = torch.full((rows, 3 * c), sentinel, dtype=dt, device="cuda")
    if precision:      # bf16 slices in y_op (pitch 3c), no f32 result
        call = lambda xx, w, bias, col, n: L.ts_conformer_linear_fwd(xx.data_ptr(), c, w.data_ptr(), frag(w), bias.data_ptr(), None, 0, None, 0,
                                                                     qkv[:, col:].data_ptr(), 3 * c, rows, n, c, act, 1, _stream())
    else:              # f32: the slice is the f32 result (pitch 3c)
        call = lambda xx, w, bias, col, n: L.ts_conformer_linear_fwd(xx.data_ptr(), c, w.data_ptr(), None, bias.data_ptr(), None, 0,
                                                                     qkv[:, col:].data_ptr(), 3 * c, None, 0, rows, n, c, act, 0, _stream())
    assert call(dxr, dwqk, dbqk, 0, 2 * c) == 0
    torch.cuda.synchronize()
    assert bool((qkv[:, 2 * c:] == sentinel).all())
    assert call(dx, dwv, dbv, 2 * c, c) == 0
    torch.cuda.synchronize()
    tol = 3e-5 if precision == 0 else 0.01

    def ref(xx, w, bias):
        z = xx.double() @ w.double().T + bias.double()
        return _act(z, act) if act else z

    want = torch.cat([ref(xr, wqk, bqk), ref(x, wv, bv)], 1)
    got = qkv.double().cpu()
    assert float((got - want).abs().max()) <= tol * float(want.abs().max())
    # FFN shape with the epilogue activation and a residual: act(x W^T + b) + res, into a buffer of its own and (the residual stream) in place
    w1, b1 = (0.1 * torch.randn(ff, c, generator=g)).to(dt), 0.1 * torch.randn(ff, generator=g)
    dw1, db1 = w1.cuda(), b1.cuda()
    h0 = torch.randn(rows, ff, generator=g)
    want = h0.double() + ref(x, w1, b1)
    res, y = h0.cuda(), torch.full((rows, ff), float("nan"), device="cuda")
    ffn = lambda out: L.ts_conformer_linear_fwd(dx.data_ptr(), c, dw1.data_ptr(), frag(dw1), db1.data_ptr(), res.data_ptr(), ff, out.data_ptr(), ff,
                                                None, 0, rows, ff, c, act, precision, _stream())
    assert ffn(y) == 0
    if precision == 0 and act:
        assert ffn(res) == _lib.TS_EUNSUPPORTED                    # f32: the activation precedes the residual, an in-place sum cannot
    else:
        assert ffn(res) == 0
    torch.cuda.synchronize()
    outs = [y] if (precision == 0 and act) else [y, res]
    for out in outs:
        assert float((out.double().cpu() - want).abs().max()) <= (3e-5 if precision == 0 else 2e-3) * float(want.abs().max())


# ---- the encoder against transformers --------------------------------------------------------------------------------------------------
def _random_conformer_ctc(family, act, seed, layers=2, **kw):
    """Every quirk visible: layer_norm_eps 1e-3 (the layers' LayerNorms and the BatchNorm keep 1e-5), random BatchNorm statistics and affine,
    biases 0.1 randn, and a nonzero positional conv that the encoder must not use."""
    torch.manual_seed(seed)
    cfg = transformers.Wav2Vec2ConformerConfig(**{**CFG, **FAMILIES[family], "hidden_act": act, "num_hidden_layers": layers, **kw})
    model = transformers.Wav2Vec2ConformerForCTC(cfg).eval()
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if k.endswith("running_mean"):
                v.copy_(0.3 * torch.randn_like(v))
            elif k.endswith("running_var"):
                v.copy_(0.5 + torch.rand_like(v))
            elif k.endswith("batch_norm.weight"):
                v.copy_(1.0 + 0.2 * torch.randn_like(v))
            elif "pos_conv_embed" in k:
                v.copy_(torch.randn_like(v))
            elif k.endswith(".bias"):
                v.copy_(0.1 * torch.randn_like(v))
    return model


def _encoder(model, precision, mask_input=False):
    from thunder_speech_amd.huggingface.compatibility import module_from_huggingface
    fe = transformers.Wav2Vec2FeatureExtractor(return_attention_mask=mask_input)
    m = module_from_huggingface(model, fe, None)
    m.encoder.precision = precision
    return m.cuda()


# bf16 bounds: test_gpu_wavlm.py's max 0.1; its rms 0.01 scaled by sqrt(23 / 12) -- a conformer layer multiplies 23 c^2 bf16 operand pairs per
# frame against a wav2vec2 layer's 12 c^2, and the independent rounding errors add in quadrature (measured up to 0.0111 with the layer-norm front end)
BF16_RMS = 0.014


def _close(got, want, precision):
    if precision == "fp32":
        np.testing.assert_allclose(got.numpy(), want.numpy(), atol=5e-4, rtol=1e-4)
    else:
        assert float((got - want).abs().max()) <= 0.1 and float((got - want).pow(2).mean().sqrt()) <= BF16_RMS, \
            (float((got - want).abs().max()), float((got - want).pow(2).mean().sqrt()))


def _run(model, x, lengths, precision, mask_input=False):
    m = _encoder(model, precision, mask_input)
    with torch.no_grad():
        h, out_len = m.encoder(x.cuda(), lengths.cuda())
    return h.transpose(1, 2).cpu(), out_len.cpu()


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("act", ["swish", "gelu"])
def test_encoder_matches_transformers(family, act):
    model = _random_conformer_ctc(family, act, seed=5)
    x = torch.randn(2, 75 * 320 + 80)
    with torch.no_grad():
        want = model.base_model(x).last_hidden_state
        pos = model.base_model.encoder.pos_conv_embed.conv
        pos.bias.add_(10.0)                                     # the positional conv is built, never called: its weights change nothing
        assert torch.equal(model.base_model(x).last_hidden_state, want)
    assert want.shape[1] == 75
    for precision in ("fp32", "bf16"):
        got, out_len = _run(model, x, torch.tensor([x.shape[1]] * 2), precision)
        assert got.shape == want.shape and out_len.tolist() == [75, 75]
        _close(got, want, precision)


def test_encoder_with_an_adapter_matches_transformers():
    model = _random_conformer_ctc("group", "swish", seed=6, add_adapter=True, num_adapter_layers=1, output_hidden_size=64)
    x = torch.randn(2, 75 * 320 + 80)
    with torch.no_grad():
        want = model.base_model(x).last_hidden_state
    assert want.shape[1:] == (38, 64)
    for precision in ("fp32", "bf16"):
        got, _ = _run(model, x, torch.tensor([x.shape[1]] * 2), precision)
        assert got.shape == want.shape
        _close(got, want, precision)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_encoder_with_ragged_lengths_matches_transformers_on_valid_frames(family):
    """Padded frames leak into a shorter clip through the depthwise conv (and from there through attention): the HIP path must compute them
    as transformers does.  A reference that zeroes the padded rows before every depthwise conv lands far from transformers on clip 1's last
    15 frames, so this test would see a kernel that masked them."""
    model = _random_conformer_ctc(family, "swish", seed=7)
    n = 75 * 320 + 80
    lengths = torch.tensor([n, 41 * 320 + 80])
    x = torch.randn(2, n)
    x[1, lengths[1]:] = 0
    mask = (torch.arange(n)[None, :] < lengths[:, None]).long()
    with torch.no_grad():
        want = model.base_model(x, attention_mask=mask).last_hidden_state
    frame_mask = (torch.arange(75)[None, :] < torch.tensor([75, 41])[:, None]).float()
    hooks = [layer.conv_module.depthwise_conv.register_forward_pre_hook(lambda mod, inp: (inp[0] * frame_mask[:, None, :],))
             for layer in model.base_model.encoder.layers]
    with torch.no_grad():
        masked = model.base_model(x, attention_mask=mask).last_hidden_state
    for hk in hooks:
        hk.remove()
    assert float((masked[1, 26:41] - want[1, 26:41]).abs().max()) >= 10 * 5e-4
    for precision in ("fp32", "bf16"):
        got, out_len = _run(model, x, lengths, precision, mask_input=True)
        assert out_len.tolist() == [75, 41]
        for i, n_i in enumerate(out_len.tolist()):
            _close(got[i, :n_i], want[i, :n_i], precision)


def test_one_layer_at_the_large_geometry():
    """1024 hidden, 16 heads, 4096 FFN, k = 31, t = 999: the published conformer-large layer."""
    model = _random_conformer_ctc("layer", "swish", seed=9, layers=1, hidden_size=1024, num_attention_heads=16, intermediate_size=4096)
    x = torch.randn(1, 999 * 320 + 80)
    with torch.no_grad():
        want = model.base_model(x).last_hidden_state
    assert want.shape[1] == 999
    for precision in ("fp32", "bf16"):
        got, _ = _run(model, x, torch.tensor([x.shape[1]]), precision)
        _close(got, want, precision)


def test_graph_replay_equals_eager_bit_for_bit():
    model = _random_conformer_ctc("group", "swish", seed=10)
    x = torch.randn(2, 60 * 320 + 80).cuda()
    lengths = torch.tensor([x.shape[1], 40 * 320]).cuda()
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


def test_a_longer_input_than_the_rotary_table_grows_it_eagerly_and_is_refused_inside_a_capture():
    model = _random_conformer_ctc("group", "gelu", seed=12, layers=1, max_source_positions=40)
    x = torch.randn(1, 60 * 320 + 80)
    with torch.no_grad():
        want = model.base_model(x).last_hidden_state
    m = _encoder(model, "fp32")
    plan = m.encoder._plan(torch.device("cuda"))
    assert plan.t_table == 40
    xs, ls = torch.randn(1, 70 * 320 + 80).cuda(), torch.tensor([70 * 320 + 80]).cuda()
    with torch.no_grad():
        graph = torch.cuda.CUDAGraph()
        with pytest.raises(RuntimeError, match="rotary table"):
            with torch.cuda.graph(graph):
                m.encoder(xs, ls)
        torch.cuda.synchronize()
    assert plan.t_table == 40
    got, _ = _run(model, x, torch.tensor([x.shape[1]]), "fp32")
    _close(got, want, "fp32")


def test_graphs_captured_before_the_rotary_table_grows_still_replay_unchanged():
    """A graph holds the rotary table's address as a launch argument.  Growing the table for a longer eager input must not free the old one:
    after the growth, small allocations that a freed table block would be handed to are made until one would cover it (or a bound is
    reached), and the graph's replay still equals its replay before the growth bit for bit."""
    model = _random_conformer_ctc("group", "swish", seed=13, layers=1, max_source_positions=40)
    enc = _encoder(model, "bf16").encoder
    dev = torch.device("cuda")
    plan = enc._plan(dev)                                               # built on the current stream: its allocator blocks belong to it
    old, nbytes = plan.cos_sin.data_ptr(), plan.cos_sin.numel() * 4
    xs, ls = torch.randn(2, 30 * 320 + 80).cuda(), torch.tensor([30 * 320 + 80] * 2).cuda()
    with torch.no_grad():
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            enc(xs, ls)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out, _ = enc(xs, ls)
        graph.replay()
        torch.cuda.synchronize()
        first = out.clone()
        xl = torch.randn(1, 60 * 320 + 80).cuda()
        enc(xl, torch.tensor([xl.shape[1]]).cuda())                    # longer than the table: grows it eagerly
        assert plan.t_table == 60 and plan.cos_sin.data_ptr() != old
        del xl
        torch.cuda.synchronize()
        junk, covered = [], False
        while len(junk) < 8192 and not covered:                        # the old table's size class, filled with a value no cos / sin has
            j = torch.full((nbytes // 4,), 1e4, device="cuda")
            junk.append(j)
            covered = j.data_ptr() < old + nbytes and old < j.data_ptr() + nbytes
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
    assert not covered, "a new allocation was handed the rotary table a captured graph still reads"
    assert torch.equal(out, first)


# ---- a saved checkpoint through the loader ---------------------------------------------------------------------------------------------
def _fit_margin_head(model, xn, margin=8.0):
    """lm_head fitted (ridge least squares on transformers' own hidden states) so that every frame's top-1 leads its top-2 by ~`margin`."""
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
    w = torch.linalg.solve(hf.T @ hf + torch.eye(c + 1, dtype=torch.float64), hf.T @ target.double())
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
    model = _random_conformer_ctc("layer", "swish", seed=11)
    g = torch.Generator().manual_seed(12)
    x = 0.1 * torch.randn(2, 30 * 320 + 80, generator=g)
    n = x.shape[1]
    xn = (x - x.mean(dim=1, keepdim=True)) / torch.sqrt(x.var(dim=1, keepdim=True, unbiased=False) + 1e-7)
    lengths = torch.tensor([n] * 2).cuda()
    am = torch.ones(2, n, dtype=torch.long)

    _save_checkpoint(model, str(tmp_path / "random_head"))
    with torch.no_grad():
        ref = model(xn, attention_mask=am).logits.transpose(1, 2)
    m = load_huggingface_checkpoint(str(tmp_path / "random_head"))
    assert m.encoder.original_encoder.config.model_type == "wav2vec2-conformer" and m.encoder.precision == "bf16" and m.encoder.mask_input
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
