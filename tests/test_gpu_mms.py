"""GPU parity of the MMS path (csrc/mms.hip and the head_dim 80 kernel of csrc/w2v_attn.hip through include/thunder_speech_amd/mms.h, then the whole encoder through the loader): the head_dim-80
attention core and the attention adapter against float64 restatements, the encoder against transformers' own Wav2Vec2 modules in f32 on the
CPU, and a two-language checkpoint directory end to end."""
import copy
import json
import math
import os

import numpy as np
import pytest
import torch

transformers = pytest.importorskip("transformers")

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t.data_ptr() if t is not None else None


# ---------------------------------------------------------------------------------------------------------------------
# 1. ts_mms_attention_fwd against float64 on the same bf16 inputs
# ---------------------------------------------------------------------------------------------------------------------
def _assert_bf16_product(got, ref, what):
    """The project's bound for this product (tests/test_gpu_w2v_kernels.py): max <= 0.03 and rms <= 0.006 of max|ref|; a NaN fails."""
    got = got.detach().double().cpu()
    assert not bool(torch.isnan(got).any()), f"{what}: unwritten (NaN) elements"
    scale = float(ref.abs().max())
    mx, rms = float((got - ref).abs().max()), float((got - ref).pow(2).mean().sqrt())
    print(f"{what}: max {mx:.3e} rms {rms:.3e} against scale {scale:.3e}")
    assert mx <= 0.03 * scale and rms <= 0.006 * scale, f"{what}: max {mx:.3e} rms {rms:.3e} against scale {scale:.3e}"


def _attention_ref(qkv, heads, n):
    """float64 softmax(q k^T / sqrt(hd)) v over the first n[b] keys; over all t keys for n <= 0."""
    b, t, c3 = qkv.shape
    c = c3 // 3
    q, k, v = [z.reshape(b, t, heads, c // heads).transpose(1, 2) for z in qkv.double().split(c, dim=-1)]
    s = (q @ k.transpose(-1, -2)) / math.sqrt(c // heads)
    lim = torch.where(n > 0, n, torch.full_like(n, t))
    s = s.masked_fill((torch.arange(t)[None, :] >= lim[:, None])[:, None, None, :], float("-inf"))
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(b, t, c)


def _run_attention(qkv, heads, key_len, ctx=None):
    from thunder_speech_amd import _lib
    b, t, c3 = qkv.shape
    c = c3 // 3
    dq, kl = qkv.cuda(), (key_len.cuda() if key_len is not None else None)
    if ctx is None:
        ctx = torch.full((b, t, c), float("nan"), dtype=BF, device="cuda")
    st = _lib.lib().ts_mms_attention_fwd(dq.data_ptr(), b, t, c, heads, _ptr(kl), ctx.data_ptr(), _stream())
    torch.cuda.synchronize()
    return st, ctx


@pytest.mark.parametrize("t", [1, 31, 32, 33, 64, 65, 128, 129, 500])
def test_attention_matches_float64(t):
    heads, c = 2, 160
    lens = [0, 1, 31, 32, 33, 63, 64, 65, t, t + 5]                          # one clip each; a length above t counts as t
    for key_len in (torch.tensor(lens, dtype=torch.int32), None):
        b = len(lens) if key_len is not None else 2
        g = torch.Generator().manual_seed(10 * t + b)
        qkv = (1.5 * torch.randn(b, t, 3 * c, generator=g)).to(BF)
        n = key_len.long().clamp(max=t) if key_len is not None else torch.full((b,), t)
        st, ctx = _run_attention(qkv, heads, key_len)
        assert st == 0
        _assert_bf16_product(ctx, _attention_ref(qkv, heads, n), f"mms attention t={t} key_len={'ragged' if key_len is not None else 'NULL'}")


def test_attention_at_the_mms_1b_geometry():
    heads, c, b, t = 16, 1280, 2, 999
    g = torch.Generator().manual_seed(77)
    qkv = (1.5 * torch.randn(b, t, 3 * c, generator=g)).to(BF)
    key_len = torch.tensor([999, 500], dtype=torch.int32)
    st, ctx = _run_attention(qkv, heads, key_len)
    assert st == 0
    _assert_bf16_product(ctx, _attention_ref(qkv, heads, key_len.long()), "mms attention 16 heads t=999")


@pytest.mark.parametrize("t", [1, 129])
def test_attention_stores_nothing_behind_the_last_row(t):
    """One head: the third 32-row block of d covers 80..95 -- the 16 elements behind the last row's 80 must keep their sentinel."""
    g = torch.Generator().manual_seed(5 + t)
    qkv = (1.5 * torch.randn(1, t, 240, generator=g)).to(BF)
    buf = torch.full((t * 80 + 16,), 7.0, dtype=BF, device="cuda")
    st, _ = _run_attention(qkv, 1, None, ctx=buf)
    assert st == 0
    assert bool((buf[t * 80:] == 7.0).all())
    _assert_bf16_product(buf[:t * 80].reshape(1, t, 80), _attention_ref(qkv, 1, torch.full((1,), t)), f"mms attention spill guard t={t}")


def test_attention_refuses_what_it_does_not_take():
    from thunder_speech_amd import _lib
    L = _lib.lib()
    qkv = torch.zeros(1, 8, 3 * 192, dtype=BF, device="cuda")
    ctx = torch.zeros(1, 8, 192, dtype=BF, device="cuda")
    call = lambda c, heads, q=qkv: L.ts_mms_attention_fwd(_ptr(q), 1, 8, c, heads, None, ctx.data_ptr(), _stream())
    assert call(128, 2) == _lib.TS_EUNSUPPORTED and call(192, 2) == _lib.TS_EUNSUPPORTED            # head_dim 64, 96
    assert call(160, 2) == 0
    assert call(160, 2, q=None) == _lib.TS_EINVAL and call(160, 3) == _lib.TS_EINVAL and call(160, 0) == _lib.TS_EINVAL
    assert L.ts_mms_attention_fwd(qkv.data_ptr() + 2, 1, 8, 160, 2, None, ctx.data_ptr(), _stream()) == _lib.TS_EUNSUPPORTED     # misaligned
    assert L.ts_mms_abi_version() == 1
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# 2. ts_mms_attn_adapter_fwd against float64
# ---------------------------------------------------------------------------------------------------------------------
SENTINEL = 12345.0
# the issue's four, then the other paths of the launcher: a half chunk at the end of the row (c % 16 == 8), a = 48 and 64 (a second k-step of
# the bf16 product), and one width per (chunks, waves) instantiation: 512, 2048, 4096
ADAPTER_SHAPES = [(1, 160, 16), (5, 160, 32), (300, 1280, 16), (37, 1024, 16), (3, 168, 16), (33, 512, 64), (40, 1280, 48), (18, 2048, 16),
                  (17, 4096, 32)]


def _adapter_case(rows, c, a, precision):
    g = torch.Generator().manual_seed(rows + c + a + precision)
    h = 2.0 * torch.randn(rows, c, generator=g) + 0.5
    nw, nb = 1.0 + 0.3 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g)
    # the adapter term of the order of h, so that a kernel that skipped it would not pass
    w1, b1 = 1.5 * torch.randn(a, c, generator=g) / math.sqrt(c), 0.3 * torch.randn(a, generator=g)
    w2, b2 = 0.5 * torch.randn(c, a, generator=g), 0.3 * torch.randn(c, generator=g)
    xw, xb = 1.0 + 0.3 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g)
    if precision:
        w1, w2 = w1.to(BF), w2.to(BF)                      # the restatement reads the same bf16-rounded weights
    hd = h.double()
    x = torch.nn.functional.layer_norm(hd, (c,), nw.double(), nb.double(), eps=1e-5)
    term = torch.relu(x @ w1.double().T + b1.double()) @ w2.double().T + b2.double()
    h_ref = hd + term
    y_ref = torch.nn.functional.layer_norm(h_ref, (c,), xw.double(), xb.double(), eps=1e-3)
    assert float(term.abs().max()) >= 0.5 * float(hd.abs().max())
    return dict(h=h, nw=nw, nb=nb, w1=w1, b1=b1, w2=w2, b2=b2, xw=xw, xb=xb, term=term, h_ref=h_ref, y_ref=y_ref)


_ADAPTER_CASES = {}


def _case(rows, c, a, precision):
    key = (rows, c, a, precision)
    if key not in _ADAPTER_CASES:
        _ADAPTER_CASES[key] = _adapter_case(*key)
    return _ADAPTER_CASES[key]


# which outputs of the fused LayerNorm are asked for: none (no LayerNorm), y_next, y_next_op, both
@pytest.mark.parametrize("precision,outs", [(0, ""), (0, "f"), (1, ""), (1, "f"), (1, "o"), (1, "fo")])
@pytest.mark.parametrize("rows,c,a", ADAPTER_SHAPES)
def test_adapter_matches_float64(rows, c, a, precision, outs):
    from thunder_speech_amd import _lib
    k = _case(rows, c, a, precision)
    d = {n: k[n].cuda() for n in ("nw", "nb", "w1", "b1", "w2", "b2", "xw", "xb")}
    hbuf = torch.full((rows + 16, c), SENTINEL, device="cuda")                # 16 rows behind the last: a workgroup's row tile must not spill
    hbuf[:rows] = k["h"].cuda()
    y = torch.full((rows, c), SENTINEL, device="cuda")
    y16 = torch.full((rows, c), SENTINEL, dtype=BF, device="cuda")
    fused = outs != ""
    # without the LayerNorm the output pointers are still passed where the precision allows them: they must stay untouched
    py = y if ("f" in outs or not fused) else None
    py16 = y16 if ("o" in outs or (not fused and precision)) else None
    st = _lib.lib().ts_mms_attn_adapter_fwd(hbuf.data_ptr(), rows, c, a, d["nw"].data_ptr(), d["nb"].data_ptr(), d["w1"].data_ptr(), d["b1"].data_ptr(),
                                            d["w2"].data_ptr(), d["b2"].data_ptr(), d["xw"].data_ptr() if fused else None,
                                            d["xb"].data_ptr() if fused else None, 1e-3, _ptr(py), _ptr(py16), precision, _stream())
    assert st == 0
    torch.cuda.synchronize()
    assert bool((hbuf[rows:] == SENTINEL).all())
    got_h = hbuf[:rows].double().cpu()
    assert not bool(torch.isnan(got_h).any())
    term_max, h_max, y_max = float(k["term"].abs().max()), float(k["h"].abs().max()), float(k["y_ref"].abs().max())
    err_h = float((got_h - k["h_ref"]).abs().max())
    bound_h = 3e-5 * float(k["h_ref"].abs().max()) if precision == 0 else 0.01 * term_max + 1e-5 * h_max
    print(f"adapter rows={rows} c={c} a={a} precision={precision} outs={outs!r}: h err {err_h:.3e} (bound {bound_h:.3e})")
    assert err_h <= bound_h, (err_h, bound_h)
    for name, buf in (("f", y), ("o", y16)):
        if name in outs:
            got = buf.double().cpu()
            assert not bool(torch.isnan(got).any())
            err = float((got - k["y_ref"]).abs().max())
            bound = (3e-5 if precision == 0 else 0.01) * y_max
            print(f"    y_next{'_op' if name == 'o' else ''} err {err:.3e} (bound {bound:.3e})")
            assert err <= bound, (name, err, bound)
        else:
            assert bool((buf == SENTINEL).all()), f"output {name!r} was not asked for and was written"


def test_adapter_refuses_what_it_does_not_take():
    from thunder_speech_amd import _lib
    L = _lib.lib()
    c = 160
    h, v = torch.zeros(4, c, device="cuda"), torch.zeros(c, device="cuda")
    w = torch.zeros(80 * c, device="cuda")
    y, y16 = torch.zeros(4, c, device="cuda"), torch.zeros(4, c, dtype=BF, device="cuda")

    def call(a=16, precision=0, next_w=None, next_b=None, yy=None, yy16=None, cc=c, hh=h, rows=4):
        return L.ts_mms_attn_adapter_fwd(_ptr(hh), rows, cc, a, v.data_ptr(), v.data_ptr(), w.data_ptr(), v.data_ptr(), w.data_ptr(), v.data_ptr(),
                                         _ptr(next_w), _ptr(next_b), 1e-5, _ptr(yy), _ptr(yy16), precision, _stream())
    assert call() == 0 and call(precision=1, next_w=v, next_b=v, yy16=y16) == 0
    assert call(a=24) == _lib.TS_EUNSUPPORTED and call(a=80) == _lib.TS_EUNSUPPORTED
    assert call(next_w=v, next_b=v, yy=y, yy16=y16) == _lib.TS_EUNSUPPORTED          # y_next_op at precision 0
    assert call(precision=2) == _lib.TS_EUNSUPPORTED and call(cc=156) == _lib.TS_EUNSUPPORTED
    assert call(next_w=v, next_b=v) == _lib.TS_EINVAL                                # a LayerNorm without an output
    assert call(next_w=v, yy=y) == _lib.TS_EINVAL                                    # next_w without next_b
    assert call(hh=None) == _lib.TS_EINVAL and call(rows=0) == _lib.TS_EINVAL and call(a=0) == _lib.TS_EINVAL
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the encoder against transformers (f32, CPU) through module_from_huggingface
# ---------------------------------------------------------------------------------------------------------------------
BASE = ["<pad>", "<s>", "</s>", "<unk>", "|"]
VOCABS = {"aaa": BASE + list("abcdefghijklmnopqrstuvwxyz'"), "bbb": BASE + list("zyxwvutsrqpo")}
# layer_norm_eps 1e-3: the adapter's own LayerNorm keeps 1e-5, and a kernel that used the config's would show
CFG = dict(hidden_size=160, num_hidden_layers=2, num_attention_heads=2, intermediate_size=320, feat_extract_norm="layer", conv_bias=True,
           do_stable_layer_norm=True, vocab_size=len(VOCABS["aaa"]), conv_dim=(32,) * 7, conv_kernel=(10, 3, 3, 3, 3, 2, 2),
           conv_stride=(5, 2, 2, 2, 2, 2, 2), num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, pad_token_id=0, adapter_attn_dim=16,
           layer_norm_eps=1e-3)
# bf16 bounds of this encoder family (tests/test_gpu_wavlm.py): max 0.1, rms 0.01.  Measured here on the full-length input of
# test_encoder_with_adapters_matches_transformers: max 0.057, rms 0.0077 (0.0083 for the same geometry without adapters), so the bound holds as it is
BF16_MAX, BF16_RMS = 0.1, 0.01


def _random_mms_ctc(seed, **kw):
    """Biases 0.1 randn everywhere; the adapters with random biases, a non-trivial norm affine and a linear_2 large enough that the adapter term
    is of the order of the residual stream (transformers initialises it near zero)."""
    torch.manual_seed(seed)
    model = transformers.Wav2Vec2ForCTC(transformers.Wav2Vec2Config(**{**CFG, **kw})).eval()
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if "adapter_layer.norm.weight" in k:
                v.copy_(1.0 + 0.3 * torch.randn_like(v))
            elif "adapter_layer.norm.bias" in k:
                v.copy_(0.2 * torch.randn_like(v))
            elif "adapter_layer.linear_1.weight" in k:
                v.copy_(1.5 * torch.randn_like(v) / math.sqrt(v.shape[1]))
            elif "adapter_layer.linear_2.weight" in k:
                v.copy_(0.5 * torch.randn_like(v))
            elif k.endswith(".bias"):
                v.copy_(0.1 * torch.randn_like(v))
    return model


def _without_adapters(model):
    bare = copy.deepcopy(model)
    for layer in bare.base_model.encoder.layers:
        layer.adapter_layer = None                         # Wav2Vec2EncoderLayerStableLayerNorm.forward: `if self.adapter_layer is not None`
    return bare


def _encoder(model, precision, mask_input=False):
    from thunder_speech_amd.huggingface.compatibility import module_from_huggingface
    fe = transformers.Wav2Vec2FeatureExtractor(return_attention_mask=mask_input)
    m = module_from_huggingface(model, fe, None)
    m.encoder.precision = precision
    return m.cuda()


def _errors(got, want):
    return float((got - want).abs().max()), float((got - want).pow(2).mean().sqrt())


def _close(got, want, precision, what=""):
    mx, rms = _errors(got, want)
    print(f"{what} {precision}: max {mx:.3e} rms {rms:.3e}")
    if precision == "fp32":
        np.testing.assert_allclose(got.numpy(), want.numpy(), atol=5e-4, rtol=1e-4)
    else:
        assert mx <= BF16_MAX and rms <= BF16_RMS, (mx, rms)


def _run(model, x, lengths, precision, mask_input=False):
    m = _encoder(model, precision, mask_input)
    with torch.no_grad():
        h, out_len = m.encoder(x.cuda(), lengths.cuda())
    return h.transpose(1, 2).cpu(), out_len.cpu(), m


@pytest.fixture(scope="module")
def small():
    """The small MMS-shaped model, one input, and transformers' outputs for it: full length, ragged, and with the adapters removed."""
    model = _random_mms_ctc(seed=31)
    g = torch.Generator().manual_seed(32)
    n = 75 * 320 + 80
    x = torch.randn(2, n, generator=g)
    lengths = torch.tensor([n, 41 * 320 + 80])
    xr = x.clone()
    xr[1, lengths[1]:] = 0
    mask = (torch.arange(n)[None, :] < lengths[:, None]).long()
    with torch.no_grad():
        full = model.base_model(x).last_hidden_state
        ragged = model.base_model(xr, attention_mask=mask).last_hidden_state
        bare = _without_adapters(model).base_model(x).last_hidden_state
    return dict(model=model, x=x, xr=xr, lengths=lengths, full=full, ragged=ragged, bare=bare)


def test_encoder_with_adapters_matches_transformers(small):
    want = small["full"]
    assert want.shape == (2, 75, 160)
    # the test can see the adapters: without them transformers lands far outside every bound below
    assert float((small["bare"] - want).abs().max()) >= 10 * BF16_MAX
    for precision in ("fp32", "bf16"):
        got, out_len, m = _run(small["model"], small["x"], torch.tensor([small["x"].shape[1]] * 2), precision)
        assert got.shape == want.shape and out_len.tolist() == [75, 75]
        plan = m.encoder._plan(torch.device("cuda"))
        assert len(plan.attn_adapter_keys) == 12 and plan.mms_attention == (precision == "bf16")
        _close(got, want, precision, "adapters, full length")


def test_encoder_with_adapters_and_ragged_lengths_matches_transformers_on_valid_frames(small):
    want = small["ragged"]
    for precision in ("fp32", "bf16"):
        got, out_len, _ = _run(small["model"], small["xr"], small["lengths"], precision, mask_input=True)
        assert out_len.tolist() == [75, 41]
        for i, n_i in enumerate(out_len.tolist()):
            _close(got[i, :n_i], want[i, :n_i], precision, f"adapters, ragged clip {i}")


def test_one_layer_at_the_mms_1b_geometry():
    """1280 hidden, 16 heads (head_dim 80), 5120 FFN, adapter 16, t = 999: one layer of facebook/mms-1b-*."""
    model = _random_mms_ctc(seed=33, num_hidden_layers=1, hidden_size=1280, num_attention_heads=16, intermediate_size=5120)
    x = torch.randn(1, 999 * 320 + 80, generator=torch.Generator().manual_seed(34))
    with torch.no_grad():
        want = model.base_model(x).last_hidden_state
        bare = _without_adapters(model).base_model(x).last_hidden_state
    assert want.shape[1] == 999 and float((bare - want).abs().max()) >= 10 * BF16_MAX
    for precision in ("fp32", "bf16"):
        got, _, _ = _run(model, x, torch.tensor([x.shape[1]]), precision)
        _close(got, want, precision, "one MMS-1B layer")


def test_head_dim_80_without_adapters_runs_fused_and_allocates_no_score_workspace():
    """XLS-R 1B's shape: head_dim 80, no adapters.  bf16 mode runs ts_mms_attention_fwd: the plan allocates no [t][t] workspace; fp32 mode does."""
    model = _random_mms_ctc(seed=35, adapter_attn_dim=None)
    assert not any("adapter_layer" in k for k in model.state_dict())
    x = torch.randn(2, 75 * 320 + 80, generator=torch.Generator().manual_seed(36))
    with torch.no_grad():
        want = model.base_model(x).last_hidden_state
    for precision in ("fp32", "bf16"):
        got, _, m = _run(model, x, torch.tensor([x.shape[1]] * 2), precision)
        _close(got, want, precision, "head_dim 80, no adapters")
        plan = m.encoder._plan(torch.device("cuda"))
        assert plan.attn_adapter_keys == []
        assert plan.mms_attention == (precision == "bf16")
        # every uint8 buffer the plan asks for during a forward: the [t][t] score workspace (2 clips x 2 heads x 75 x 75 x 4 bytes in fp32 mode,
        # x 6 with the bf16 copy of the probabilities) is requested on the materialised path only
        asked, buf = [], plan._buf
        plan._buf = lambda *shape, dtype=torch.float32: (asked.append(shape[0]) if dtype == torch.uint8 else None, buf(*shape, dtype=dtype))[1]
        with torch.no_grad():
            m.encoder(x.cuda(), torch.tensor([x.shape[1]] * 2).cuda())
        torch.cuda.synchronize()
        plan._buf = buf
        scores = 2 * 2 * 75 * 75
        if precision == "bf16":
            assert scores * 6 not in asked and scores * 4 not in asked, asked
        else:
            assert scores * 4 in asked, asked


def test_graph_replay_equals_eager_bit_for_bit(small):
    x = small["xr"].cuda()
    lengths = small["lengths"].cuda()
    enc = _encoder(small["model"], "bf16", mask_input=True).encoder
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


# ---- a saved two-language checkpoint through the loader ------------------------------------------------------------------------------------
def _fit_margin_head(model, xn, n_tokens, margin=8.0):
    """lm_head fitted (ridge least squares on transformers' own hidden states) so that every frame's top-1 leads its top-2 by ~`margin`
    (tests/test_gpu_conformer.py's, for a vocabulary of n_tokens)."""
    with torch.no_grad():
        h = model.base_model(xn).last_hidden_state
    b, t, c = h.shape
    labels = torch.zeros(b, t, dtype=torch.long)
    for i in range(b):
        for f in range(t):
            labels[i, f] = 0 if (f // 3) % 2 else 5 + (3 * i + f // 6) % (n_tokens - 5)
    target = torch.full((b * t, n_tokens), -margin / 2)
    target[torch.arange(b * t), labels.reshape(-1)] = margin / 2
    hf = torch.cat([h.reshape(b * t, c), torch.ones(b * t, 1)], 1).double()
    # ridge 1e-3: 60 frames against 161 unknowns fit the targets almost exactly (with the conformer test's 1.0 these hidden states leave margins of 0.4)
    w = torch.linalg.solve(hf.T @ hf + 1e-3 * torch.eye(c + 1, dtype=torch.float64), hf.T @ target.double())
    with torch.no_grad():
        model.lm_head.weight.copy_(w[:c].T.float())
        model.lm_head.bias.copy_(w[c].float())


def test_two_language_checkpoint_loads_the_target_language_and_predicts(tmp_path):
    from safetensors.torch import save_file
    from thunder_speech_amd.huggingface.compatibility import load_huggingface_checkpoint
    from thunder_speech_amd.module import greedy_decode
    g = torch.Generator().manual_seed(42)
    x = 0.1 * torch.randn(2, 30 * 320 + 80, generator=g)
    n = x.shape[1]
    xn = (x - x.mean(dim=1, keepdim=True)) / torch.sqrt(x.var(dim=1, keepdim=True, unbiased=False) + 1e-7)
    am = torch.ones(2, n, dtype=torch.long)
    # the network of language "bbb": its own adapters and a margin head on its own vocabulary
    second = _random_mms_ctc(seed=41, vocab_size=len(VOCABS["bbb"]))
    _fit_margin_head(second, xn, len(VOCABS["bbb"]))
    # the directory holds the shared weights with language "aaa"'s adapters and head; each language's adapter file next to them
    first = _random_mms_ctc(seed=43)
    shared = {k: v for k, v in second.state_dict().items() if "adapter_layer" not in k and not k.startswith("lm_head")}
    first.load_state_dict(shared, strict=False)
    d = str(tmp_path / "mms")
    first.save_pretrained(d)
    for lang, model in (("aaa", first), ("bbb", second)):
        save_file({k: v.detach().clone().contiguous() for k, v in model._get_adapters().items()}, os.path.join(d, f"adapter.{lang}.safetensors"))
    with open(os.path.join(d, "vocab.json"), "w") as f:
        json.dump({lang: {tok: i for i, tok in enumerate(toks)} for lang, toks in VOCABS.items()}, f)
    transformers.Wav2Vec2CTCTokenizer(os.path.join(d, "vocab.json"), target_lang="aaa").save_pretrained(d)
    transformers.Wav2Vec2FeatureExtractor(return_attention_mask=True).save_pretrained(d)

    with torch.no_grad():
        ref = second(xn, attention_mask=am).logits.transpose(1, 2)
    top2 = ref.topk(2, dim=1).values
    assert float((top2[:, 0] - top2[:, 1]).min()) > 0.5 * max(1.0, float(ref.abs().max()))
    m = load_huggingface_checkpoint(d, target_lang="bbb")
    assert m.decoder[2].weight.shape == (len(VOCABS["bbb"]), 160) and m.text_transform.num_tokens == len(VOCABS["bbb"])
    assert torch.equal(m.encoder.original_encoder.encoder.layers[1].adapter_layer.linear_2.weight,
                       second.base_model.encoder.layers[1].adapter_layer.linear_2.weight)
    assert m.encoder.precision == "bf16" and m.encoder.mask_input
    m = m.cuda()
    m.graph_inference = True
    xc = x.cuda()                                                       # one address: predict()'s zero-copy graph is keyed by it
    lengths = torch.tensor([n] * 2).cuda()
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
