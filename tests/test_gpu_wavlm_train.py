"""GPU parity of WavLM FINE-TUNING in mixed precision (csrc/wavlm_train.hip through include/thunder_speech_amd/wavlm_train.h, then the training path
of huggingface/train.py): the kernels against a float64 restatement of transformers' WavLMAttention, the gate and the embedding gradient against
float64 autograd of transformers' own modules, and whole encoders against transformers' f32 autograd on the CPU."""
import json
import os

import numpy as np
import pytest
import torch

transformers = pytest.importorskip("transformers")

pytestmark = pytest.mark.gpu

VOCAB = ["<pad>", "<s>", "</s>", "<unk>", "|"] + list("abcdefghijklmnopqrstuvwxyz'")
CFG = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, vocab_size=len(VOCAB), conv_dim=(32, 32, 32),
           conv_stride=(5, 2, 2), conv_kernel=(10, 3, 2), num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=2, hidden_dropout=0.0,
           activation_dropout=0.0, attention_dropout=0.0, feat_proj_dropout=0.0, final_dropout=0.0, layerdrop=0.0, mask_time_prob=0.0,
           mask_feature_prob=0.0, num_buckets=32, max_bucket_distance=40, pad_token_id=0)
FAMILIES = {"base": dict(feat_extract_norm="group", do_stable_layer_norm=False, conv_bias=False),
            "large": dict(feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True)}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rel(a, r):
    return float((a.double() - r.double()).norm() / r.double().norm())


# ---------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------
def _keep_mask(b, heads, t, p, seed):
    """ts_train_dropout's keep decisions over the logical [B H t][t] matrix (ones in, kept elements nonzero out)."""
    from thunder_speech_amd import _lib
    ones = torch.ones(b * heads * t, t, device="cuda")
    out = torch.empty_like(ones)
    assert _lib.lib().ts_train_dropout(ones.data_ptr(), out.data_ptr(), b * heads * t, t, t, float(p), int(seed), None, 0, _stream()) == 0
    return (out != 0).view(b, heads, t, t)


def _diag_index(t):
    return torch.arange(t)[None, :] - torch.arange(t)[:, None] + t - 1          # [i][j] -> j - i + t - 1


def _reference(q16, g, rb, key_len, heads, p, keep, dout):
    """float64 restatement on the bf16-rounded q / k / v; returns ctx and the gradients of q, k, v, g, rb."""
    b, t, c3 = q16.shape
    c = c3 // 3
    qkv = q16.double().detach().requires_grad_(True)
    g = g.double().detach().requires_grad_(True)
    rb = rb.double().detach().requires_grad_(True)
    q, k, v = [z.reshape(b, t, heads, 64).transpose(1, 2) for z in qkv.split(c, dim=-1)]
    s = (q @ k.transpose(-1, -2)) / 8.0 + g[..., None] * rb[:, _diag_index(t).to(rb.device)][None]
    n = torch.full((b,), t, device=s.device) if key_len is None else key_len.long().clamp(max=t)
    pad = torch.arange(t, device=s.device)[None, :] >= n[:, None]
    s = s.masked_fill((pad & (n[:, None] > 0))[:, None, None, :], float("-inf"))
    prob = torch.softmax(s, -1) * (n > 0).double()[:, None, None, None]          # key_len <= 0: probability 0 everywhere
    if p > 0:
        prob = prob * keep.double() / (1.0 - p)
    ctx = (prob @ v).transpose(1, 2).reshape(b, t, c)
    ctx.backward(dout.double())
    return ctx.detach(), qkv.grad, g.grad, rb.grad


def _lse2(q16, g, rb, key_len, heads, dtype):
    """log2(sum over the valid keys of exp(q k / 8 + gate rel_bias)) in `dtype` on the CPU, [B][H][t]; -inf for a clip without a valid key."""
    b, t, c3 = q16.shape
    c = c3 // 3
    q, k = [z.reshape(b, t, heads, 64).transpose(1, 2) for z in q16.cpu().to(dtype).split(c, dim=-1)[:2]]
    s = (q @ k.transpose(-1, -2)) / 8.0 + g.cpu().to(dtype)[..., None] * rb.cpu().to(dtype)[:, _diag_index(t)][None]
    n = torch.full((b,), t) if key_len is None else key_len.cpu().long().clamp(max=t)
    s = s.masked_fill((torch.arange(t)[None, :] >= n[:, None])[:, None, None, :], float("-inf"))
    return torch.logsumexp(s, -1) / float(np.log(2.0)), n


def _run(q16, g, rb, key_len, heads, p, seed, dout):
    """ts_wavlm_attention_train_fwd / _bwd with every output filled with NaN first."""
    from thunder_speech_amd import _lib
    L = _lib.lib()
    b, t, c3 = q16.shape
    c = c3 // 3
    kl = key_len.data_ptr() if key_len is not None else None
    ctx = torch.full((b, t, c), float("nan"), device="cuda")
    lse2 = torch.full((b, heads, t), float("nan"), device="cuda")
    wsf = torch.empty(L.ts_wavlm_attention_train_fwd_workspace(b, t, c, heads), dtype=torch.uint8, device="cuda")
    assert L.ts_wavlm_attention_train_fwd(q16.data_ptr(), b, t, c, heads, kl, p, seed, g.data_ptr(), rb.data_ptr(), ctx.data_ptr(), lse2.data_ptr(),
                                          wsf.data_ptr(), _stream()) == 0
    dqkv = torch.full((b, t, c3), float("nan"), device="cuda")
    dg = torch.full_like(g, float("nan"))
    drb = torch.full_like(rb, float("nan"))
    ws = torch.empty(L.ts_wavlm_attention_train_bwd_workspace(b, t, c, heads), dtype=torch.uint8, device="cuda")
    assert L.ts_wavlm_attention_train_bwd(q16.data_ptr(), b, t, c, heads, kl, p, seed, g.data_ptr(), rb.data_ptr(), dout.data_ptr(), ctx.data_ptr(),
                                          lse2.data_ptr(), wsf.data_ptr() if p > 0 else None, dqkv.data_ptr(), dg.data_ptr(), drb.data_ptr(),
                                          ws.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    return ctx, lse2, dqkv, dg, drb


def _inputs(b, t, heads, seed):
    torch.manual_seed(seed)
    c = 64 * heads
    q16 = (torch.randn(b, t, 3 * c, device="cuda") * 1.5).to(torch.bfloat16)
    g = 1.0 + 1.5 * torch.rand(b, heads, t, device="cuda")                       # the gate's range is (1, 3) for c near 1
    rb = 1.5 * torch.randn(heads, 2 * t - 1, device="cuda")
    dout = torch.randn(b, t, c, device="cuda")
    return q16, g, rb, dout


@pytest.mark.parametrize("b,t,heads,p,ragged", [(2, 1, 1, 0.0, False), (2, 33, 2, 0.1, True), (3, 130, 2, 0.0, True), (1, 130, 4, 0.1, False),
                                                (2, 499, 2, 0.1, True), (2, 499, 1, 0.0, False), (1, 900, 2, 0.0, False), (2, 900, 1, 0.1, True)])
def test_fused_attention_kernels_match_a_float64_restatement(b, t, heads, p, ragged):
    """ctx, dq, dk, dv, dgate and drel_bias within 2e-2 relative L2 (bf16 operands), dropout mask = ts_train_dropout's for the same seed, frame
    counts off the 64 / 128 tiles and beyond max_distance, ragged key lengths with a clip at 0, every output element written."""
    q16, g, rb, dout = _inputs(b, t, heads, b * 1000 + t + heads)
    key_len = torch.tensor([t, 0, max(t // 2, 1)][:b], dtype=torch.int32, device="cuda") if ragged else None
    seed = 20240917
    keep = _keep_mask(b, heads, t, p, seed) if p > 0 else None
    ctx, lse2, dqkv, dg, drb = _run(q16, g, rb, key_len, heads, p, seed, dout)
    for x in (ctx, dqkv, dg, drb):
        assert bool(torch.isfinite(x).all())
    assert not bool(torch.isnan(lse2).any())
    # the row statistic the backward rebuilds every probability from: f32 arithmetic on bf16 operands, so within 4 x the error of the same expression in
    # float32 on the CPU (floor 1e-5 x max |lse2|); a clip without a valid key holds +inf (every rebuilt probability exp2(s - inf) is 0)
    want, n = _lse2(q16, g, rb, key_len, heads, torch.float64)
    some = n > 0
    own = float((_lse2(q16, g, rb, key_len, heads, torch.float32)[0].double() - want)[some].abs().max())
    err = float((lse2.double().cpu() - want)[some].abs().max())
    print(f"lse2 b={b} t={t}: error {err:.3e}, float32 on the CPU {own:.3e}")
    assert err <= max(4.0 * own, 1e-5 * float(want[some].abs().max())), (err, own)
    assert bool((lse2.cpu()[~some] == float("inf")).all())
    rctx, rdqkv, rdg, rdrb = _reference(q16, g, rb, key_len, heads, p, keep, dout)
    c = 64 * heads

    def close(got, ref):
        # t = 1: one key per row, so dS = P (dP - D) = 0 and dq, dk, dg, drb vanish in exact arithmetic; in mixed precision they hold the bf16
        # rounding of dP against the f32 row dot D, measured against the scale of the gradients that do not vanish (dv)
        if float(ref.norm()) > 1e-6 * float(rctx.norm()):
            return _rel(got, ref) <= 2e-2
        return float(got.norm()) <= 2e-2 * float(rdqkv[..., 2 * c:].norm())
    assert close(ctx, rctx)
    for sl in (slice(0, c), slice(c, 2 * c), slice(2 * c, 3 * c)):
        assert close(dqkv[..., sl], rdqkv[..., sl])
    assert close(dg, rdg)
    assert close(drb, rdrb)
    if ragged:                                           # the clip without a valid key: no output, no gradient
        assert float(ctx[1].abs().max()) == 0.0 and float(dqkv[1].abs().max()) == 0.0 and float(dg[1].abs().max()) == 0.0
    if p > 0:
        other = _run(q16, g, rb, key_len, heads, p, seed + 1, dout)
        assert _rel(other[0], rctx) > 5e-2


def test_fused_attention_is_reproducible_bit_for_bit():
    q16, g, rb, dout = _inputs(2, 300, 2, 3)
    key_len = torch.tensor([300, 211], dtype=torch.int32, device="cuda")
    r1 = _run(q16, g, rb, key_len, 2, 0.1, 42, dout)
    r2 = _run(q16, g, rb, key_len, 2, 0.1, 42, dout)
    for x, y in zip(r1, r2):
        assert torch.equal(x, y)


def test_gate_forward_and_backward_match_transformers_in_float64():
    from transformers.models.wavlm.modeling_wavlm import WavLMAttention
    from thunder_speech_amd import _lib
    L = _lib.lib()
    b, t, heads = 3, 77, 4
    torch.manual_seed(11)
    att = WavLMAttention(64 * heads, heads).double()
    with torch.no_grad():
        att.gru_rel_pos_linear.weight.copy_(0.2 * torch.randn(8, 64))
        att.gru_rel_pos_linear.bias.copy_(0.5 * torch.randn(8))
        att.gru_rel_pos_const.copy_(1.0 + 0.5 * torch.randn(1, heads, 1, 1))
    x = torch.randn(b, t, 64 * heads, dtype=torch.float64, requires_grad=True)
    # WavLMAttention.forward steps 1-3, on the module's own parameters
    gh = x.view(b, t, heads, -1).permute(0, 2, 1, 3)
    proj = att.gru_rel_pos_linear(gh).view(gh.shape[:-1] + (2, 4)).sum(-1)
    ga, gb = torch.sigmoid(proj).chunk(2, dim=-1)
    want = (ga * (gb * att.gru_rel_pos_const - 1.0) + 2.0).squeeze(-1)          # [b][H][t]
    dg = torch.randn(b, heads, t, dtype=torch.float64)
    want.backward(dg)
    f = lambda z: z.detach().float().contiguous().cuda()
    xg, w, bias, cst = f(x), f(att.gru_rel_pos_linear.weight), f(att.gru_rel_pos_linear.bias), f(att.gru_rel_pos_const.view(-1))
    gate = torch.full((b, heads, t), float("nan"), device="cuda")
    gab = torch.empty(2, b, heads, t, device="cuda")
    assert L.ts_wavlm_gate_fwd(xg.data_ptr(), b, t, heads, 64 * heads, w.data_ptr(), bias.data_ptr(), cst.data_ptr(), gate.data_ptr(), gab.data_ptr(),
                               _stream()) == 0
    dx = torch.full_like(xg, float("nan"))
    dw, db, dc = torch.full_like(w, float("nan")), torch.full_like(bias, float("nan")), torch.full_like(cst, float("nan"))
    ws = torch.empty(L.ts_wavlm_gate_bwd_workspace(b, t, heads), dtype=torch.uint8, device="cuda")
    dgc = f(dg)
    assert L.ts_wavlm_gate_bwd(xg.data_ptr(), b, t, heads, 64 * heads, w.data_ptr(), cst.data_ptr(), gab.data_ptr(), dgc.data_ptr(), dx.data_ptr(),
                               dw.data_ptr(), db.data_ptr(), dc.data_ptr(), ws.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    for got, ref in ((gate, want), (dx, x.grad), (dw, att.gru_rel_pos_linear.weight.grad), (db, att.gru_rel_pos_linear.bias.grad),
                     (dc, att.gru_rel_pos_const.grad.view(-1))):
        assert _rel(got.cpu(), ref.detach()) <= 1e-4


@pytest.mark.parametrize("nb,md,t", [(320, 800, 1), (320, 800, 499), (320, 800, 900), (32, 40, 130)])
def test_embedding_gradient_matches_compute_bias_autograd(nb, md, t):
    """d rel_attn_embed through compute_bias (float64 autograd) for an upstream gradient on the diagonals; buckets no diagonal reaches get 0."""
    from transformers.models.wavlm.modeling_wavlm import WavLMAttention
    from thunder_speech_amd import _lib
    from thunder_speech_amd.huggingface.encoder import wavlm_bucket_table
    heads = 4
    torch.manual_seed(t)
    att = WavLMAttention(64 * heads, heads, num_buckets=nb, max_distance=md).double()
    values = att.compute_bias(t, t)                                               # [H][t][t]
    d = torch.arange(2 * t - 1) - (t - 1)
    rows = (-d).clamp(min=0)
    rb = values[:, rows, rows + d]                                                # [H][2t - 1] diagonals
    drb = torch.randn(heads, 2 * t - 1, dtype=torch.float64)
    (rb * drb).sum().backward()
    want = att.rel_attn_embed.weight.grad
    table = wavlm_bucket_table(nb, md).cuda()
    de = torch.full((nb, heads), float("nan"), device="cuda")
    drbc = drb.float().contiguous().cuda()
    assert _lib.lib().ts_wavlm_rel_bias_bwd(drbc.data_ptr(), table.data_ptr(), nb, md, heads, t, de.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(de).all())
    assert _rel(de.cpu(), want) <= 1e-4
    assert torch.equal(de.cpu() == 0, want == 0)


# ---------------------------------------------------------------------------------------------------------------------
# the training path against transformers
# ---------------------------------------------------------------------------------------------------------------------
def _model(family, seed=0, **over):
    torch.manual_seed(seed)
    m = transformers.WavLMModel(transformers.WavLMConfig(**{**CFG, **FAMILIES[family], **over}))
    with torch.no_grad():                       # make every parameter matter, the WavLM-only ones included
        for n, p in m.named_parameters():
            if p.dim() == 1 and "bias" in n:
                p.add_(0.05 * torch.randn_like(p))
            elif "layer_norm.weight" in n:
                p.mul_(1.0 + 0.1 * torch.randn_like(p))
            elif n.endswith("rel_attn_embed.weight"):
                p.copy_(1.5 * torch.randn_like(p))
            elif n.endswith("gru_rel_pos_const"):
                p.copy_(1.0 + 0.5 * torch.randn_like(p))
            elif n.endswith("gru_rel_pos_linear.weight"):
                p.copy_(0.1 * torch.randn_like(p))
        if hasattr(m, "masked_spec_embed"):
            m.masked_spec_embed.copy_(torch.randn_like(m.masked_spec_embed))
    return m


def _pair(family, seed=0, **over):
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    ref = _model(family, seed, **over)
    ref.freeze_feature_encoder()
    ref.train()
    mine = _model(family, seed, **over)
    mine.load_state_dict(ref.state_dict())
    adapt = HuggingFaceEncoderAdapt(mine, precision="fp32", train_precision="bf16").cuda().train()
    return ref, adapt


def _audio(b=3, n=4000, seed=1):
    return torch.randn(b, n, generator=torch.Generator().manual_seed(seed))


GATE_TOL = 1e-1     # gru_rel_pos_linear.* / gru_rel_pos_const: sums over every (clip, frame) of dg = sum_j dS rb, rows whose terms cancel, so
                    # the bf16 rounding of dS shows more there (measured 1.5e-2 .. 8.5e-2 on these models); likewise k_proj.bias, whose true
                    # gradient is 0 (a per-row shift of the logits) and is measured against the floor (4.1e-2 measured); every other gradient: 4e-2


def _compare_grads(ref, adapt, tol=4e-2):
    mine = dict(adapt.original_encoder.named_parameters())
    floor = 1e-4 * max(float(p.grad.norm()) for p in ref.parameters() if p.grad is not None)
    checked = set()
    rels = {n: float((mine[n].grad.cpu() - p.grad).norm()) / max(float(p.grad.norm()), floor) for n, p in ref.named_parameters()
            if p.requires_grad and p.grad is not None and mine[n].grad is not None}
    print("relative L2 of the gradients:", sorted(rels.items(), key=lambda kv: -kv[1])[:8])
    for name, p in ref.named_parameters():
        q = mine[name]
        if not p.requires_grad:
            assert q.grad is None or float(q.grad.abs().max()) == 0.0, name
            continue
        if p.grad is None:                                  # a LayerDrop-skipped layer: no gradient on either side
            assert q.grad is None or float(q.grad.abs().max()) == 0.0, name
            continue
        assert q.grad is not None, name
        rel = float((q.grad.cpu() - p.grad).norm()) / max(float(p.grad.norm()), floor)
        assert rel <= (GATE_TOL if ("gru_rel_pos" in name or name.endswith("k_proj.bias")) else tol), (name, rel)
        checked.add(name)
    return checked


def _graph_names(out):
    seen, todo = set(), [out.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        todo += [f for f, _ in fn.next_functions]
    return [type(fn).__name__ for fn in seen]


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("masked", [False, True])
def test_training_forward_and_every_gradient_match_transformers_autograd(family, masked):
    """All dropouts off: last_hidden_state within 3e-2 of its scale and the gradient of EVERY trainable parameter within 4e-2 relative L2 (the bf16
    bar of the wav2vec2 path) -- rel_attn_embed.weight, gru_rel_pos_linear.* and gru_rel_pos_const included."""
    ref, adapt = _pair(family)
    adapt.mask_input = masked
    x = _audio()
    lengths = torch.tensor([4000, 3000, 2111])
    att = None
    if masked:
        x = x * (torch.arange(x.shape[1])[None, :] < lengths[:, None])
        att = (torch.arange(x.shape[1])[None, :] < lengths[:, None]).long()
    out_ref = ref(x, attention_mask=att).last_hidden_state
    probe = torch.randn(out_ref.shape, generator=torch.Generator().manual_seed(5))
    (out_ref * probe).sum().backward()
    feats, _ = adapt(x.cuda(), lengths.cuda())
    got = feats.transpose(-1, -2)
    err = float((got.detach().cpu() - out_ref.detach()).abs().max())
    assert err <= 3e-2 * max(1.0, float(out_ref.abs().max())), err
    names = _graph_names(got)
    assert names.count("WavLMAttentionFusedBackward") == 2 and "WavLMGateBackward" in names and names.count("WavLMRelBiasBackward") == 1
    (got * probe.cuda()).sum().backward()
    checked = _compare_grads(ref, adapt)
    assert {"encoder.layers.0.attention.rel_attn_embed.weight", "encoder.layers.0.attention.gru_rel_pos_linear.weight",
            "encoder.layers.1.attention.gru_rel_pos_linear.bias", "encoder.layers.1.attention.gru_rel_pos_const"} <= checked
    assert len(checked) > 30


def test_training_is_reproducible_bit_for_bit():
    """The forward and the gradients of the WavLM-only parameters: no atomics on their path (the wav2vec2 nodes' bias gradients add with atomics)."""
    _, adapt = _pair("large")
    adapt.mask_input = True
    x = _audio(b=2, n=6000, seed=4).cuda()
    lengths = torch.tensor([6000, 4100]).cuda()
    probe = None
    res = []
    for _ in range(2):
        adapt.zero_grad(set_to_none=True)
        feats, _ = adapt(x, lengths)
        probe = torch.randn(feats.shape, generator=torch.Generator().manual_seed(9)).cuda() if probe is None else probe
        (feats * probe).sum().backward()
        res.append([feats.detach().clone()] + [p.grad.clone() for n, p in adapt.original_encoder.named_parameters()
                                               if "gru_rel_pos" in n or "rel_attn_embed" in n])
    assert len(res[0]) == len(res[1]) == 8
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_layerdrop_never_skips_layer_zero_and_keeps_the_torch_rng_in_step():
    ref, adapt = _pair("base", layerdrop=1.0, num_hidden_layers=4)
    x = _audio(b=2, n=3000, seed=3)
    torch.manual_seed(21)
    out_ref = ref(x).last_hidden_state
    after_ref = torch.rand([])
    torch.manual_seed(21)
    feats, _ = adapt(x.cuda(), torch.tensor([3000, 3000]).cuda())
    after = torch.rand([])
    assert torch.equal(after, after_ref)
    got = feats.transpose(-1, -2)
    assert _graph_names(got).count("WavLMAttentionFusedBackward") == 1           # layer 0 only
    err = float((got.detach().cpu() - out_ref.detach()).abs().max())
    assert err <= 3e-2 * max(1.0, float(out_ref.abs().max())), err


def test_time_masking_follows_transformers_under_the_same_numpy_seed():
    ref, adapt = _pair("base", mask_time_prob=0.3, mask_time_length=3, mask_time_min_masks=2)
    x = _audio(b=2, n=6000, seed=2)
    np.random.seed(11)
    out_ref = ref(x).last_hidden_state
    probe = torch.randn(out_ref.shape, generator=torch.Generator().manual_seed(6))
    (out_ref * probe).sum().backward()
    np.random.seed(11)
    feats, _ = adapt(x.cuda(), torch.tensor([6000, 6000]).cuda())
    got = feats.transpose(-1, -2)
    err = float((got.detach().cpu() - out_ref.detach()).abs().max())
    assert err <= 3e-2 * max(1.0, float(out_ref.abs().max())), err
    (got * probe.cuda()).sum().backward()
    checked = _compare_grads(ref, adapt)
    assert "masked_spec_embed" in checked


def test_dropouts_are_random_and_differentiable():
    _, adapt = _pair("large", hidden_dropout=0.1, activation_dropout=0.1, attention_dropout=0.1, feat_proj_dropout=0.1)
    x = _audio(b=2, n=4000, seed=8).cuda()
    a, _ = adapt(x, torch.tensor([4000, 4000]).cuda())
    b_, _ = adapt(x, torch.tensor([4000, 4000]).cuda())
    assert not torch.equal(a, b_)
    a.sum().backward()
    for n, p in adapt.original_encoder.named_parameters():
        if p.requires_grad and p.grad is not None:
            assert bool(torch.isfinite(p.grad).all()), n


def test_ctc_training_steps_through_the_module_train_the_wavlm_parameters(tmp_path):
    """module_from_huggingface on a tiny WavLMForCTC, train_precision="bf16", three AdamW steps of BaseCTCModule.training_step: the loss falls,
    every gradient is finite, rel_attn_embed and the gate parameters move, the frozen feature extractor does not."""
    from thunder_speech_amd.huggingface.compatibility import module_from_huggingface
    d = str(tmp_path)
    with open(os.path.join(d, "vocab.json"), "w") as f:
        json.dump({tok: i for i, tok in enumerate(VOCAB)}, f)
    tok = transformers.Wav2Vec2CTCTokenizer(os.path.join(d, "vocab.json"))
    torch.manual_seed(3)
    model = transformers.WavLMForCTC(transformers.WavLMConfig(**{**CFG, **FAMILIES["base"]}))
    module = module_from_huggingface(model, transformers.Wav2Vec2FeatureExtractor(return_attention_mask=True), tok)
    module.encoder.train_precision = "bf16"
    module.optimizer_kwargs = {"lr": 1e-3}
    module = module.cuda().train()
    enc = module.encoder.original_encoder
    before = {n: p.detach().clone() for n, p in enc.named_parameters()}
    opt = module.configure_optimizers()
    batch = (_audio(b=2, n=8000, seed=7).cuda(), torch.tensor([8000.0, 6000.0]).cuda(), ["hello world", "abc"])
    losses = []
    for _ in range(4):
        opt.zero_grad()
        loss = module.training_step(batch, 0)
        loss.backward()
        for n, p in module.named_parameters():
            if p.grad is not None:
                assert bool(torch.isfinite(p.grad).all()), n
        opt.step()
        losses.append(float(loss))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    moved = {n: float((p.detach() - before[n]).abs().max()) for n, p in enc.named_parameters()}
    assert all(v == 0.0 for n, v in moved.items() if n.startswith("feature_extractor."))
    for n in ("encoder.layers.0.attention.rel_attn_embed.weight", "encoder.layers.0.attention.gru_rel_pos_linear.weight",
              "encoder.layers.1.attention.gru_rel_pos_linear.bias", "encoder.layers.1.attention.gru_rel_pos_const"):
        assert moved[n] > 0, n
