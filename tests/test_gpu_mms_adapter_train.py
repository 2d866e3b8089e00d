"""GPU parity of adapter-only MMS fine-tuning (csrc/mms_adapter_train.hip through include/thunder_speech_amd/mms_adapter_train.h, then
huggingface/train.py's AttnAdapter node): the out-of-place forward and the fused backward against float64 autograd, the whole model against
transformers' autograd with the base frozen, and one optimizer step through BaseCTCModule.training_step."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SENTINEL = 12345.0
SHAPES = [(1, 160, 16),        # one row of a 16-row tile
          (5, 160, 32),
          (3, 168, 16),        # c % 16 == 8
          (37, 1024, 16),
          (33, 512, 64),       # a second k-step, rows % 16 == 1
          (40, 1280, 48),
          (17, 4096, 32),      # the widest row
          (300, 1280, 16)]     # many tiles for the reductions over rows
# max-norm error of a gradient relative to max|reference|: f32 products -- the bound tests/test_gpu_w2v_kernels.py gives ts_w2v_layernorm_bwd;
# bf16 operands -- the project's bound for gradients from bf16 operands (tests/test_gpu_mms_train.py)
GRAD_BOUND = {0: 1e-5, 1: 2e-2}
MARGIN = 0.02
GRADS = ("dh", "d_nw", "d_nb", "d_w1", "d_b1", "d_w2", "d_b2")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _adapter_case(rows, c, a, precision):
    """Inputs scaled as tests/test_gpu_mms.py::_adapter_case, plus dy; float64 autograd on the CPU is the reference.  A ReLU decision within
    rounding noise of zero would flip and let the reference itself miss any bound, so every row of h with a unit |z| < MARGIN rms(z) is redrawn."""
    g = torch.Generator().manual_seed(rows + c + a + precision)
    h = 2.0 * torch.randn(rows, c, generator=g) + 0.5
    nw, nb = 1.0 + 0.3 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g)
    w1, b1 = 1.5 * torch.randn(a, c, generator=g) / math.sqrt(c), 0.3 * torch.randn(a, generator=g)
    w2, b2 = 0.5 * torch.randn(c, a, generator=g), 0.3 * torch.randn(c, generator=g)
    dy = torch.randn(rows, c, generator=g)
    if precision:
        w1, w2 = w1.to(BF), w2.to(BF)                      # the reference reads the same bf16-rounded weights

    def z_of(hh):
        return torch.nn.functional.layer_norm(hh.double(), (c,), nw.double(), nb.double(), eps=1e-5) @ w1.double().T + b1.double()
    redraws = 0
    while True:
        z = z_of(h)
        rms = float(z.pow(2).mean().sqrt())
        bad = (z.abs() < MARGIN * rms).any(dim=1)
        if not bool(bad.any()):
            break
        n = int(bad.sum())
        redraws += n
        assert redraws <= 1000, "the ReLU margin does not converge"
        h[bad] = 2.0 * torch.randn(n, c, generator=g) + 0.5
    assert float(z.abs().min()) >= MARGIN * rms
    leaves = [t.double().clone().requires_grad_(True) for t in (h, nw, nb, w1, b1, w2, b2)]
    hd, nwd, nbd, w1d, b1d, w2d, b2d = leaves
    term = torch.relu(torch.nn.functional.layer_norm(hd, (c,), nwd, nbd, eps=1e-5) @ w1d.T + b1d) @ w2d.T + b2d
    y = hd + term
    (y * dy.double()).sum().backward()
    assert float(term.detach().abs().max()) >= 0.5 * float(hd.detach().abs().max())
    ref = dict(zip(GRADS, (t.grad for t in leaves)))
    ref["dh"] = ref["dh"] - dy.double()                    # the adapter's share: the identity part must not hide it
    return dict(h=h, nw=nw, nb=nb, w1=w1, b1=b1, w2=w2, b2=b2, dy=dy, term=term.detach(), y_ref=y.detach(), ref=ref, redraws=redraws)


_CASES = {}


def _case(rows, c, a, precision):
    key = (rows, c, a, precision)
    if key not in _CASES:
        _CASES[key] = _adapter_case(*key)
    return _CASES[key]


def _dev(k):
    return {n: k[n].cuda() for n in ("h", "nw", "nb", "w1", "b1", "w2", "b2", "dy")}


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _backward(d, rows, c, a, precision, want_dh=True):
    """-> (dh or None, the six parameter gradients, the status); every buffer and the workspace pre-filled with NaN, 16 sentinel rows behind dh."""
    from thunder_speech_amd import _lib
    L = _lib.lib()
    dh = None
    if want_dh:
        dh = torch.full((rows + 16, c), SENTINEL, device="cuda")
        dh[:rows] = float("nan")
    out = [_nan(c), _nan(c), _nan(a, c), _nan(a), _nan(c, a), _nan(c)]
    nbytes = L.ts_mms_attn_adapter_train_bwd_workspace(rows, c, a)
    assert nbytes > 0 and nbytes % 4 == 0
    ws = _nan(nbytes // 4)
    st = L.ts_mms_attn_adapter_train_bwd(d["h"].data_ptr(), d["dy"].data_ptr(), rows, c, a, d["nw"].data_ptr(), d["nb"].data_ptr(), d["w1"].data_ptr(),
                                         d["b1"].data_ptr(), d["w2"].data_ptr(), _ptr(dh), *(t.data_ptr() for t in out), ws.data_ptr(), precision,
                                         _stream())
    torch.cuda.synchronize()
    return dh, out, st


def _check_backward(rows, c, a, precision):
    k = _case(rows, c, a, precision)
    d = _dev(k)
    h0 = d["h"].clone()
    dh, out, st = _backward(d, rows, c, a, precision)
    assert st == 0
    assert bool((dh[rows:] == SENTINEL).all()) and torch.equal(d["h"], h0)
    got = dict(zip(GRADS, [dh[:rows].double().cpu() - k["dy"].double()] + [t.double().cpu() for t in out]))
    errs = {}
    for name in GRADS:
        assert not bool(torch.isnan(got[name]).any()), f"{name}: unwritten (NaN) elements"
        errs[name] = float((got[name] - k["ref"][name]).abs().max()) / float(k["ref"][name].abs().max())
    print(f"adapter bwd rows={rows} c={c} a={a} precision={precision} (redrawn rows {k['redraws']}): " +
          " ".join(f"{n} {e:.2e}" for n, e in errs.items()) + f" (bound {GRAD_BOUND[precision]:.0e})")
    for name, e in errs.items():
        assert e <= GRAD_BOUND[precision], (name, e)
    # dh = NULL (no upstream gradient wanted): the six parameter gradients, bit for bit
    _, out2, st = _backward(d, rows, c, a, precision, want_dh=False)
    assert st == 0
    for name, t1, t2 in zip(GRADS[1:], out, out2):
        assert torch.equal(t1, t2), name


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("rows,c,a", SHAPES)
def test_forward_matches_float64_and_the_in_place_kernel(rows, c, a, precision):
    from thunder_speech_amd import _lib
    L = _lib.lib()
    k = _case(rows, c, a, precision)
    d = _dev(k)
    h0 = d["h"].clone()
    y = torch.full((rows + 16, c), SENTINEL, device="cuda")
    y[:rows] = float("nan")
    st = L.ts_mms_attn_adapter_train_fwd(d["h"].data_ptr(), rows, c, a, d["nw"].data_ptr(), d["nb"].data_ptr(), d["w1"].data_ptr(), d["b1"].data_ptr(),
                                         d["w2"].data_ptr(), d["b2"].data_ptr(), y.data_ptr(), precision, _stream())
    assert st == 0
    inplace = d["h"].clone()
    st = L.ts_mms_attn_adapter_fwd(inplace.data_ptr(), rows, c, a, d["nw"].data_ptr(), d["nb"].data_ptr(), d["w1"].data_ptr(), d["b1"].data_ptr(),
                                   d["w2"].data_ptr(), d["b2"].data_ptr(), None, None, 1e-5, None, None, precision, _stream())
    assert st == 0
    torch.cuda.synchronize()
    assert torch.equal(d["h"], h0) and bool((y[rows:] == SENTINEL).all())
    got = y[:rows].double().cpu()
    assert not bool(torch.isnan(got).any())
    err = float((got - k["y_ref"]).abs().max())
    bound = 3e-5 * float(k["y_ref"].abs().max()) if precision == 0 else 0.01 * float(k["term"].abs().max()) + 1e-5 * float(k["h"].abs().max())
    print(f"adapter train fwd rows={rows} c={c} a={a} precision={precision}: y err {err:.3e} (bound {bound:.3e})")
    assert err <= bound, (err, bound)
    assert torch.equal(y[:rows], inplace)


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("rows,c,a", SHAPES)
def test_backward_matches_float64_autograd(rows, c, a, precision):
    _check_backward(rows, c, a, precision)


@pytest.mark.parametrize("precision", [0, 1])
def test_two_runs_give_the_same_bits(precision):
    rows, c, a = 300, 1280, 16
    d = _dev(_case(rows, c, a, precision))
    dh1, out1, _ = _backward(d, rows, c, a, precision)
    dh2, out2, _ = _backward(d, rows, c, a, precision)
    assert torch.equal(dh1, dh2) and not bool(torch.isnan(dh1).any())
    for t1, t2 in zip(out1, out2):
        assert torch.equal(t1, t2) and not bool(torch.isnan(t1).any())


def test_one_call_at_the_mms_1b_row_geometry():
    _check_backward(2 * 499, 1280, 16, 1)


def test_entry_points_refuse_what_they_do_not_take():
    from thunder_speech_amd import _lib
    L = _lib.lib()
    assert L.ts_mms_adapter_train_abi_version() == 1
    c, rows = 160, 4
    h, v, w = torch.zeros(rows, c, device="cuda"), torch.zeros(c, device="cuda"), torch.zeros(80 * c, device="cuda")
    y = torch.zeros(rows, c, device="cuda")
    ws = torch.zeros(1 << 20, device="cuda")
    EINVAL, EUNSUP = _lib.TS_EINVAL, _lib.TS_EUNSUPPORTED

    def fwd(a=16, precision=0, cc=c, rr=rows, **over):
        p = dict(h=h, nw=v, nb=v, w1=w, b1=v, w2=w, b2=v, y=y)
        p.update(over)
        ptr = {n: (t if isinstance(t, int) else _ptr(t)) for n, t in p.items()}
        return L.ts_mms_attn_adapter_train_fwd(ptr["h"], rr, cc, a, ptr["nw"], ptr["nb"], ptr["w1"], ptr["b1"], ptr["w2"], ptr["b2"], ptr["y"],
                                               precision, _stream())

    def bwd(a=16, precision=0, cc=c, rr=rows, **over):
        p = dict(h=h, dy=y, nw=v, nb=v, w1=w, b1=v, w2=w, dh=y, d_nw=v, d_nb=v, d_w1=w, d_b1=v, d_w2=w, d_b2=v, ws=ws)
        p.update(over)
        ptr = {n: (t if isinstance(t, int) else _ptr(t)) for n, t in p.items()}
        return L.ts_mms_attn_adapter_train_bwd(ptr["h"], ptr["dy"], rr, cc, a, ptr["nw"], ptr["nb"], ptr["w1"], ptr["b1"], ptr["w2"], ptr["dh"],
                                               ptr["d_nw"], ptr["d_nb"], ptr["d_w1"], ptr["d_b1"], ptr["d_w2"], ptr["d_b2"], ptr["ws"], precision,
                                               _stream())
    assert fwd() == 0 and fwd(precision=1) == 0 and bwd() == 0 and bwd(precision=1) == 0 and bwd(dh=None) == 0
    for call, required in ((fwd, ("h", "nw", "nb", "w1", "b1", "w2", "b2", "y")),
                           (bwd, ("h", "dy", "nw", "nb", "w1", "b1", "w2", "d_nw", "d_nb", "d_w1", "d_b1", "d_w2", "d_b2", "ws"))):
        for name in required:
            assert call(**{name: None}) == EINVAL, name
        assert call(rr=0) == EINVAL and call(cc=0) == EINVAL and call(a=0) == EINVAL and call(rr=-1) == EINVAL
        assert call(a=24) == EUNSUP and call(a=80) == EUNSUP and call(cc=156) == EUNSUP and call(cc=4104) == EUNSUP
        assert call(precision=2) == EUNSUP and call(precision=-1) == EUNSUP
        for name in required + (("dh",) if call is bwd else ()):
            assert call(**{name: h.data_ptr() + 4}) == EUNSUP, name                    # 4-byte aligned only
    W = L.ts_mms_attn_adapter_train_bwd_workspace
    assert W(0, c, 16) == EINVAL and W(rows, 0, 16) == EINVAL and W(rows, c, 0) == EINVAL and W(rows, c, 16) > 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# the whole model against transformers' autograd, the base frozen
# ---------------------------------------------------------------------------------------------------------------------
# tests/test_gpu_mms_train.py's BASE in its pre-LN family, with attention adapters
CFG = dict(vocab_size=32, hidden_size=160, num_hidden_layers=2, num_attention_heads=2, intermediate_size=320, conv_dim=(32, 32, 32),
           conv_stride=(5, 2, 2), conv_kernel=(10, 3, 2), num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, hidden_dropout=0.0,
           activation_dropout=0.0, attention_dropout=0.0, feat_proj_dropout=0.0, final_dropout=0.0, layerdrop=0.0, mask_time_prob=0.0,
           mask_feature_prob=0.0, feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True, adapter_attn_dim=16)


def _model(transformers, seed=0):
    torch.manual_seed(seed)
    m = transformers.Wav2Vec2Model(transformers.Wav2Vec2Config(**CFG))
    with torch.no_grad():
        for n, p in m.named_parameters():       # tests/test_gpu_mms_train.py::_model: make every parameter matter
            if p.dim() == 1 and "bias" in n:
                p.add_(0.05 * torch.randn_like(p))
            elif "layer_norm.weight" in n:
                p.mul_(1.0 + 0.1 * torch.randn_like(p))
        for k, v in m.state_dict().items():     # tests/test_gpu_mms.py::_random_mms_ctc: the adapter term of the order of the residual stream
            if "adapter_layer.norm.weight" in k:
                v.copy_(1.0 + 0.3 * torch.randn_like(v))
            elif "adapter_layer.norm.bias" in k:
                v.copy_(0.2 * torch.randn_like(v))
            elif "adapter_layer.linear_1.weight" in k:
                v.copy_(1.5 * torch.randn_like(v) / math.sqrt(v.shape[1]))
            elif "adapter_layer.linear_2.weight" in k:
                v.copy_(0.5 * torch.randn_like(v))
            elif "adapter_layer" in k and k.endswith(".bias"):
                v.copy_(0.1 * torch.randn_like(v))
    return m


def _clips():
    x = torch.randn(3, 4000, generator=torch.Generator().manual_seed(1))
    lengths = torch.tensor([4000, 3000, 2111])
    valid = torch.arange(x.shape[1])[None, :] < lengths[:, None]
    return x * valid, lengths, valid.long()


def _far_biases(model, x, att):
    """linear_1.bias = +-3 x the rms of linear_1's output, alternating by unit, layer by layer: upstream bf16 noise of about 1 % of z then flips
    almost no ReLU decision (with ordinary biases transformers in bf16 would itself miss the bound on linear_1's gradient)."""
    for layer in model.encoder.layers:
        lin = layer.adapter_layer.linear_1
        seen = []
        with torch.no_grad():
            lin.bias.zero_()
            hook = lin.register_forward_hook(lambda mod, inp, out: seen.append(out.detach()))
            model(x, attention_mask=att)
            hook.remove()
            rms = float(seen[0].pow(2).mean().sqrt())
            lin.bias.copy_(3.0 * rms * (1.0 - 2.0 * (torch.arange(lin.bias.numel()) % 2)))


def _graph(fn):
    seen, todo = set(), [fn]
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        todo += [g for g, _ in f.next_functions]
    return seen


@pytest.mark.parametrize("train_precision", ["fp32", "bf16"])
def test_whole_model_matches_transformers_autograd_with_the_base_frozen(train_precision):
    transformers = pytest.importorskip("transformers")
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    x, lengths, att = _clips()
    ref = _model(transformers)
    ref.train()
    if train_precision == "bf16":
        _far_biases(ref, x, att)
    mine = _model(transformers)
    mine.load_state_dict(ref.state_dict())
    # the reference in the same regime, by hand
    for n, p in ref.named_parameters():
        p.requires_grad_(".adapter_layer." in n)
    adapt = HuggingFaceEncoderAdapt(mine, mask_input=True, precision="fp32", train_precision=train_precision).cuda().train()
    named = adapt.adapter_finetuning()
    assert len(named) == 12

    out_ref = ref(x, attention_mask=att).last_hidden_state
    probe = torch.randn(out_ref.shape, generator=torch.Generator().manual_seed(5))
    (out_ref * probe).sum().backward()
    feats, _ = adapt(x.cuda(), lengths.cuda())
    got = feats.transpose(-1, -2)
    err = float((got.detach().cpu() - out_ref.detach()).abs().max())
    print(f"{train_precision}: output max abs error {err:.3e} against scale {float(out_ref.detach().abs().max()):.3e}")
    if train_precision == "fp32":
        np.testing.assert_allclose(got.detach().cpu().numpy(), out_ref.detach().numpy(), atol=5e-4, rtol=1e-4)
    else:
        assert err <= 3e-2 * max(1.0, float(out_ref.detach().abs().max())), err
        assert err > 1e-6, "the mixed-precision path did not run"

    nodes = _graph(got.grad_fn)
    names = {type(f).__name__ for f in nodes}
    assert "AttnAdapterBackward" in names, names
    if train_precision == "bf16":
        assert "AttentionFused80Backward" in names and "AttentionBackward" not in names, names
    else:
        assert "AttentionBackward" in names, names
    params = {id(p): n for n, p in named.items()}
    leaves = {params.get(id(f.variable)) for f in nodes if type(f).__name__ == "AccumulateGrad"}
    assert None not in leaves and leaves == set(named), leaves                # the graph ends in the adapter parameters and nothing else
    first = [f for f in nodes if type(f).__name__ == "AttnAdapterBackward" and f.next_functions[0][0] is None]
    assert len(first) == 1                                                    # the first layer's adapter: nothing below it but its parameters
    assert {params[id(g.variable)] for g, _ in first[0].next_functions[1:]} == {n for n in named if ".layers.0." in n}

    (got * probe.cuda()).sum().backward()
    theirs = dict(adapt.original_encoder.named_parameters())
    floor = 1e-4 * max(float(p.grad.norm()) for p in ref.parameters() if p.grad is not None)
    bound = 1e-3 if train_precision == "fp32" else 4e-2
    checked = 0
    for name, p in ref.named_parameters():
        q = theirs[name]
        if not p.requires_grad:
            assert q.grad is None and not q.requires_grad, name
            continue
        assert p.grad is not None and q.grad is not None, name
        r = float((q.grad.cpu() - p.grad).norm()) / max(float(p.grad.norm()), floor)
        print(f"    {name}: relative gradient error {r:.3e}")
        assert r <= bound, (name, r)
        checked += 1
    assert checked == 12
    if train_precision == "fp32":                                             # ordinary biases: the ReLU mask is exercised both ways
        z = []
        hook = ref.encoder.layers[0].adapter_layer.linear_1.register_forward_hook(lambda mod, inp, out: z.append(out.detach()))
        with torch.no_grad():
            ref(x, attention_mask=att)
        hook.remove()
        frac = float((z[0] > 0).float().mean())
        assert 0.2 < frac < 0.8, frac
    with torch.no_grad():
        feats2, _ = adapt(x.cuda(), lengths.cuda())
    assert torch.equal(feats2, feats)


def test_one_optimizer_step_trains_the_adapters_and_the_head_only():
    transformers = pytest.importorskip("transformers")
    from thunder_speech_amd.blocks import linear_decoder
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    from thunder_speech_amd.huggingface.transform import Wav2Vec2Preprocess
    from thunder_speech_amd.module import BaseCTCModule
    from thunder_speech_amd.text_processing.transform import BatchTextTransformer
    enc = HuggingFaceEncoderAdapt(_model(transformers, seed=3), precision="fp32", train_precision="bf16")
    named = enc.adapter_finetuning()
    tokens = [chr(97 + i) for i in range(26)] + [" "]
    module = BaseCTCModule(enc, linear_decoder(160, len(tokens) + 1, 0.0), Wav2Vec2Preprocess(), BatchTextTransformer(tokens=tokens),
                           optimizer_kwargs={"lr": 1e-3}).cuda()
    opt = module.configure_optimizers()
    assert isinstance(opt, torch.optim.AdamW)
    trained = {id(p) for group in opt.param_groups for p in group["params"]}
    assert trained == {id(p) for p in named.values()} | {id(p) for p in module.decoder.parameters()}
    x = torch.randn(2, 8000, generator=torch.Generator().manual_seed(7)).cuda()
    lengths = torch.tensor([8000, 8000]).cuda()
    module.eval()
    with torch.no_grad():
        logits0, _ = module(x, lengths)
    before = {n: p.detach().clone() for n, p in enc.named_parameters()}
    head = {n: p.detach().clone() for n, p in module.decoder.named_parameters()}
    module.train()
    opt.zero_grad()
    loss = module.training_step((x, torch.tensor([8000.0, 6000.0]).cuda(), ["hello world", "abc"]), 0)
    loss.backward()
    opt.step()
    assert math.isfinite(float(loss))
    for n, p in enc.named_parameters():
        if n in named:
            assert p.grad is not None and not torch.equal(p.detach(), before[n]), n
        else:
            assert p.grad is None and torch.equal(p.detach(), before[n]), n
    assert all(not torch.equal(p.detach(), head[n]) for n, p in module.decoder.named_parameters())
    module.eval()
    with torch.no_grad():
        texts = module.predict(x)
        logits1, _ = module(x, lengths)
    assert len(texts) == 2 and all(isinstance(t, str) for t in texts)
    assert logits1.shape == logits0.shape and bool(torch.isfinite(logits1.float()).all()) and not torch.equal(logits1, logits0)
    # the encoder's own output moved too: the inference plan was re-packed from the stepped adapter weights
    with torch.no_grad():
        f1, _ = enc(x, lengths)
        for n, p in enc.named_parameters():
            p.copy_(before[n])
        f0, _ = enc(x, lengths)
    assert not torch.equal(f1, f0)
