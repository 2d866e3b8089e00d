"""GPU parity of head_dim 80 fine-tuning (csrc/mms_train.hip and the head_dim 80 kernels of csrc/w2v_attn_train.hip through include/thunder_speech_amd/mms_train.h, then huggingface/train.py's
AttentionFused80): the fused training attention against float64 (forward, row statistic, and float64 autograd for dq / dk / dv under the oracle's
Philox keep mask), against the materialised f32 `Attention` node, and a whole head_dim 80 Wav2Vec2Model against transformers' autograd on the CPU.

Bounds, all the project's: a bf16 product (tests/test_gpu_mms.py: max <= 0.03, rms <= 0.006 of max|ref|), gradients of the attention core
(tests/test_gpu_w2v_train.py: relative L2 <= 2e-2), the whole model in mixed precision (same file: output within 3e-2 of its scale, every
parameter gradient <= 4e-2 relative L2)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
HD = 80
LOG2E = 1.4426950408889634


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _assert_bf16_product(got, ref, what):
    """max <= 0.03 and rms <= 0.006 of max|ref|; a NaN fails."""
    got = got.detach().double().cpu()
    assert not bool(torch.isnan(got).any()), f"{what}: unwritten (NaN) elements"
    scale = float(ref.abs().max())
    mx, rms = float((got - ref).abs().max()), float((got - ref).pow(2).mean().sqrt())
    print(f"{what}: max {mx:.3e} rms {rms:.3e} against scale {scale:.3e}")
    assert mx <= 0.03 * scale and rms <= 0.006 * scale, f"{what}: max {mx:.3e} rms {rms:.3e} against scale {scale:.3e}"


def _rel(a, r):
    return float((a.double().cpu() - r.double().cpu()).norm() / r.double().cpu().norm())


def _limits(key_len, b, t):
    """Valid keys per clip, the training convention: NULL = t, <= 0 = none, above t = t."""
    if key_len is None:
        return torch.full((b,), t, dtype=torch.long)
    return key_len.long().clamp(min=0, max=t)


def _reference(qkv, heads, key_len, keep=None, p=0.0):
    """float64 on the CPU: ctx [B][t][c], lse2 [B][H][t] (+inf without a valid key) and the leaf q64 to take gradients through.
    keep: bool [B][H][t][t] or None."""
    b, t, c3 = qkv.shape
    c = c3 // 3
    x = qkv.double().cpu().clone().requires_grad_(True)
    q, k, v = [z.reshape(b, t, heads, HD).transpose(1, 2) for z in x.split(c, dim=-1)]
    s = (q @ k.transpose(-1, -2)) / math.sqrt(HD)
    valid = (torch.arange(t)[None, :] < _limits(key_len, b, t)[:, None])[:, None, None, :]            # [B][1][1][t]
    # a row without a valid key: every probability 0 (the softmax over a constant row times the all-false mask)
    prob = torch.softmax(s.masked_fill(~valid, -1e300), -1) * valid
    lse2 = torch.logsumexp(s.detach().masked_fill(~valid, float("-inf")), -1) * LOG2E
    lse2 = torch.where(valid.any(-1).expand(b, heads, t), lse2, torch.full_like(lse2, float("inf")))
    if keep is not None:
        prob = prob * keep.double() / (1.0 - p)
    ctx = (prob @ v).transpose(1, 2).reshape(b, t, c)
    return x, ctx, lse2


def _forward(q16, heads, key_len, p=0.0, seed=0, ctx=None):
    from thunder_speech_amd import _lib
    L = _lib.lib()
    b, t, c3 = q16.shape
    c = c3 // 3
    if ctx is None:
        ctx = torch.full((b, t, c), float("nan"), device="cuda")
    lse2 = torch.full((b, heads, t), float("nan"), device="cuda")
    ws = torch.empty(L.ts_mms_attention_train_fwd_workspace(b, t, c, heads), dtype=torch.uint8, device="cuda") if p > 0 else None
    st = L.ts_mms_attention_train_fwd(q16.data_ptr(), b, t, c, heads, _ptr(key_len), p, seed, ctx.data_ptr(), lse2.data_ptr(), _ptr(ws), _stream())
    torch.cuda.synchronize()
    assert st == 0
    return ctx, lse2, ws


def _backward(q16, heads, key_len, p, seed, dout, ctx, lse2, fwd_mask, dqkv=None):
    from thunder_speech_amd import _lib
    L = _lib.lib()
    b, t, c3 = q16.shape
    c = c3 // 3
    if dqkv is None:
        dqkv = torch.full((b, t, c3), float("nan"), device="cuda")
    ws = torch.empty(L.ts_mms_attention_train_bwd_workspace(b, t, c, heads), dtype=torch.uint8, device="cuda")
    st = L.ts_mms_attention_train_bwd(q16.data_ptr(), b, t, c, heads, _ptr(key_len), p, seed, dout.data_ptr(), ctx.data_ptr(), lse2.data_ptr(),
                                      _ptr(fwd_mask), dqkv.data_ptr(), ws.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert st == 0
    return dqkv


def _qkv(b, t, heads, seed):
    g = torch.Generator().manual_seed(seed)
    return (1.5 * torch.randn(b, t, 3 * HD * heads, generator=g)).to(BF)


# ---------------------------------------------------------------------------------------------------------------------
# 1. forward against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [1, 31, 33, 64, 65, 129, 200])
def test_forward_matches_float64(t):
    heads = 2
    lens = [0, 1, 31, 32, 33, 63, 64, 65, t, t + 5]                          # one clip each; a length above t counts as t, 0 = no valid key
    for key_len in (torch.tensor(lens, dtype=torch.int32), None):
        b = len(lens) if key_len is not None else 2
        qkv = _qkv(b, t, heads, 10 * t + b)
        _, ref, lse_ref = _reference(qkv, heads, key_len)
        ctx, lse2, _ = _forward(qkv.cuda(), heads, key_len.cuda() if key_len is not None else None)
        what = f"mms train forward t={t} key_len={'ragged' if key_len is not None else 'NULL'}"
        _assert_bf16_product(ctx, ref.detach(), what)
        lse2 = lse2.double().cpu()
        some = torch.isfinite(lse_ref)
        err = float((lse2[some] - lse_ref[some]).abs().max())
        print(f"{what}: lse2 max abs error {err:.3e}")
        assert err <= 1e-3
        assert bool((lse2[~some] == float("inf")).all())
        if key_len is not None:
            assert not bool(some[0].any()) and bool(some[1:].all())
            assert float(ctx[0].abs().max()) == 0.0                          # the clip with no valid key: exactly zero


# ---------------------------------------------------------------------------------------------------------------------
# 2. backward against float64 autograd under the oracle's keep mask
# ---------------------------------------------------------------------------------------------------------------------
def _key_len(b, t, ragged):
    return torch.tensor(([t, t // 2, 0] * 2)[:b], dtype=torch.int32) if ragged else None


@pytest.mark.parametrize("b,t,heads,p,ragged", [(2, 130, 2, 0.0, False), (3, 129, 2, 0.1, True), (1, 33, 1, 0.5, False), (2, 200, 2, 0.25, True)])
def test_backward_matches_float64_autograd(b, t, heads, p, ragged):
    from oracle import philox as ph
    c = HD * heads
    seed = 987654321012345
    qkv = _qkv(b, t, heads, 1000 * b + t)
    key_len = _key_len(b, t, ragged)
    dout = torch.randn(b, t, c, generator=torch.Generator().manual_seed(t))
    keep = torch.from_numpy(ph.dropout_keep(seed, b * heads * t * t, p)).view(b, heads, t, t) if p > 0 else None
    x, ref, _ = _reference(qkv, heads, key_len, keep, p)
    (ref * dout.double()).sum().backward()
    kl = key_len.cuda() if key_len is not None else None
    ctx, lse2, mask = _forward(qkv.cuda(), heads, kl, p, seed)
    _assert_bf16_product(ctx, ref.detach(), f"mms train forward under dropout p={p}")
    dqkv = _backward(qkv.cuda(), heads, kl, p, seed, dout.cuda(), ctx, lse2, mask)
    assert bool(torch.isfinite(dqkv).all()), "dqkv: unwritten (NaN) elements"
    for name, sl in (("dq", slice(0, c)), ("dk", slice(c, 2 * c)), ("dv", slice(2 * c, 3 * c))):
        r = _rel(dqkv[..., sl], x.grad[..., sl])
        print(f"{name} b={b} t={t} heads={heads} p={p} ragged={ragged}: relative L2 {r:.3e}")
        assert r <= 2e-2, (name, r)
    if ragged:                                           # the clip with no valid key (b = 3 has one): zero context, zero gradients
        none = [i for i, n in enumerate(key_len.tolist()) if n <= 0]
        assert bool(none) == (b >= 3) and all(float(dqkv[i].abs().max()) == 0.0 and float(ctx[i].abs().max()) == 0.0 for i in none)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the kept and the re-drawn mask; two whole runs
# ---------------------------------------------------------------------------------------------------------------------
def test_kept_and_redrawn_mask_and_two_whole_runs_give_the_same_bits():
    b, t, heads, p, seed = 2, 211, 3, 0.2, 77
    qkv = _qkv(b, t, heads, 2).cuda()
    key_len = torch.tensor([t, 100], dtype=torch.int32, device="cuda")
    dout = torch.randn(b, t, HD * heads, generator=torch.Generator().manual_seed(3)).cuda()
    runs = []
    for _ in range(2):
        ctx, lse2, mask = _forward(qkv, heads, key_len, p, seed)
        kept = _backward(qkv, heads, key_len, p, seed, dout, ctx, lse2, mask)
        redrawn = _backward(qkv, heads, key_len, p, seed, dout, ctx, lse2, None)
        assert torch.equal(kept, redrawn) and bool(torch.isfinite(kept).all())
        runs.append((ctx, lse2, kept))
    for x0, x1 in zip(*runs):
        assert torch.equal(x0, x1)


# ---------------------------------------------------------------------------------------------------------------------
# 4. nothing is stored behind the last row
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [1, 129])
def test_nothing_is_stored_behind_the_last_row(t):
    """One head: the third 32-row block of d covers 80..95 -- the 16 floats behind the last row of ctx and of dqkv must keep their sentinel."""
    qkv = _qkv(1, t, 1, 5 + t)
    dout = torch.randn(1, t, HD, generator=torch.Generator().manual_seed(t))
    x, ref, _ = _reference(qkv, 1, None)
    (ref * dout.double()).sum().backward()
    cbuf = torch.full((t * HD + 16,), 7.0, device="cuda")
    gbuf = torch.full((t * 3 * HD + 16,), 7.0, device="cuda")
    ctx, lse2, _ = _forward(qkv.cuda(), 1, None, ctx=cbuf)
    _backward(qkv.cuda(), 1, None, 0.0, 0, dout.cuda(), ctx, lse2, None, dqkv=gbuf)
    assert bool((cbuf[t * HD:] == 7.0).all()) and bool((gbuf[t * 3 * HD:] == 7.0).all())
    _assert_bf16_product(cbuf[:t * HD].reshape(1, t, HD), ref.detach(), f"mms train spill guard t={t}")
    dqkv = gbuf[:t * 3 * HD].reshape(1, t, 3 * HD)
    assert bool(torch.isfinite(dqkv).all()) and not bool((dqkv == 7.0).all(-1).any())
    for name, sl in (("dq", slice(0, HD)), ("dk", slice(HD, 2 * HD)), ("dv", slice(2 * HD, 3 * HD))):
        if t == 1 and name != "dv":
            # one key: the probability is 1 whatever q and k are, so dq = dk = 0 in float64 and a relative error has no meaning.  The kernel's
            # dS = dP - D is the rounding residue of dO to bf16 (relative 2^-9 per element; D is summed from the f32 dO), doubled for the f32 sums:
            # |dS| <= 2^-8 sum_d |dO_d v_d|, and dq = dS k / sqrt(80), dk = dS q / sqrt(80)
            q64, k64, v64 = qkv.double().split(HD, dim=-1)
            ds = 2.0 ** -8 * float((dout.double() * v64).abs().sum())
            assert float(dqkv[..., sl].abs().max()) <= ds * float((k64 if name == "dq" else q64).abs().max()) / math.sqrt(HD), name
            continue
        assert _rel(dqkv[..., sl], x.grad[..., sl]) <= 2e-2, name


# ---------------------------------------------------------------------------------------------------------------------
# 5. through train.attention() in mixed mode, against the materialised f32 node
# ---------------------------------------------------------------------------------------------------------------------
def _against_the_materialised_node(b, t, heads, p, key_len):
    from thunder_speech_amd.huggingface import train as T
    torch.manual_seed(b * 100 + t)
    c = HD * heads
    qkv = (torch.randn(b, t, 3 * c, device="cuda") * 1.5).requires_grad_(True)
    seed = 987654321012345
    ref = T.Attention.apply(qkv, key_len, heads, p, seed)
    dout = torch.randn_like(ref)
    ref.backward(dout)
    dref = qkv.grad.clone()
    qkv.grad = None
    with T.mixed_precision(True):
        out = T.attention(qkv, key_len, heads, p, seed)
        assert isinstance(out.grad_fn, T.AttentionFused80._backward_cls) and type(out.grad_fn).__name__ == "AttentionFused80Backward"
        out.backward(dout)
        other = T.attention(qkv.detach(), key_len, heads, p, seed + 1) if p > 0 else None
    torch.cuda.synchronize()
    assert _rel(out.detach(), ref.detach()) <= 2e-2
    for sl in (slice(0, c), slice(c, 2 * c), slice(2 * c, 3 * c)):
        assert bool(torch.isfinite(qkv.grad[..., sl]).all())
        assert _rel(qkv.grad[..., sl], dref[..., sl]) <= 2e-2
    if other is not None:                                # the mask matters: another seed gives another result
        assert _rel(other, ref.detach()) > 5e-2


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("ragged", [False, True])
def test_attention_node_matches_the_materialised_path(p, ragged):
    b, t, heads = 3, 130, 2
    _against_the_materialised_node(b, t, heads, p, torch.tensor([t, t // 2, 0], dtype=torch.int32, device="cuda") if ragged else None)


def test_the_switch_still_selects_the_materialised_node():
    from thunder_speech_amd.huggingface import train as T
    qkv = torch.randn(1, 40, 3 * 160, device="cuda", requires_grad=True)
    old_f = T.FUSED_ATTENTION
    try:
        T.FUSED_ATTENTION = False
        with T.mixed_precision(True):
            assert isinstance(T.attention(qkv, None, 2, 0.0, 0).grad_fn, T.Attention._backward_cls)
        T.FUSED_ATTENTION = True                                          # f32 training is unchanged
        with T.mixed_precision(False):
            assert isinstance(T.attention(qkv, None, 2, 0.0, 0).grad_fn, T.Attention._backward_cls)
    finally:
        T.FUSED_ATTENTION = old_f


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_what_they_do_not_take():
    from thunder_speech_amd import _lib
    L = _lib.lib()
    b, t = 1, 8
    qkv = torch.zeros(b, t, 3 * 192, dtype=BF, device="cuda")
    ctx, lse2 = torch.zeros(b, t, 192, device="cuda"), torch.zeros(b, 4, t, device="cuda")
    dout, dqkv = torch.zeros(b, t, 192, device="cuda"), torch.zeros(b, t, 3 * 192, device="cuda")
    ws = torch.empty(max(L.ts_mms_attention_train_bwd_workspace(b, t, 192, 2), 16), dtype=torch.uint8, device="cuda")

    def fwd(c, heads, q=qkv.data_ptr(), p=0.0):
        return L.ts_mms_attention_train_fwd(q, b, t, c, heads, None, p, 1, ctx.data_ptr(), lse2.data_ptr(), ws.data_ptr(), _stream())

    def bwd(c, heads, q=qkv.data_ptr(), p=0.0):
        return L.ts_mms_attention_train_bwd(q, b, t, c, heads, None, p, 1, dout.data_ptr(), ctx.data_ptr(), lse2.data_ptr(), None, dqkv.data_ptr(),
                                            ws.data_ptr(), _stream())

    for call in (fwd, bwd):
        assert call(128, 2) == _lib.TS_EUNSUPPORTED and call(192, 2) == _lib.TS_EUNSUPPORTED            # head_dim 64, 96
        assert call(160, 2, q=qkv.data_ptr() + 2) == _lib.TS_EUNSUPPORTED                               # misaligned
        assert call(160, 2, q=None) == _lib.TS_EINVAL and call(160, 0) == _lib.TS_EINVAL and call(160, 3) == _lib.TS_EINVAL
        assert call(160, 2, p=1.0) == _lib.TS_EINVAL and call(160, 2, p=-0.1) == _lib.TS_EINVAL
        assert call(160, 2) == 0 and call(160, 2, p=0.5) == 0
    assert L.ts_mms_attention_train_fwd(qkv.data_ptr(), b, t, 160, 2, None, 0.0, 1, None, lse2.data_ptr(), None, _stream()) == _lib.TS_EINVAL
    assert L.ts_mms_attention_train_fwd(qkv.data_ptr(), b, t, 160, 2, None, 0.5, 1, ctx.data_ptr(), lse2.data_ptr(), None, _stream()) == _lib.TS_EINVAL
    assert L.ts_mms_attention_train_fwd_workspace(0, t, 160, 2) == _lib.TS_EINVAL and L.ts_mms_attention_train_bwd_workspace(b, t, 160, 0) == _lib.TS_EINVAL
    assert L.ts_mms_train_abi_version() == 1
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# 7. one call at the 1B head geometry
# ---------------------------------------------------------------------------------------------------------------------
def test_one_call_at_the_xls_r_1b_head_geometry():
    _against_the_materialised_node(2, 499, 16, 0.1, torch.tensor([499, 250], dtype=torch.int32, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------------
# 8. a whole head_dim 80 model against transformers' autograd
# ---------------------------------------------------------------------------------------------------------------------
BASE = dict(vocab_size=32, hidden_size=160, num_hidden_layers=2, num_attention_heads=2, intermediate_size=320, conv_dim=(32, 32, 32),
            conv_stride=(5, 2, 2), conv_kernel=(10, 3, 2), num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, hidden_dropout=0.0,
            activation_dropout=0.0, attention_dropout=0.0, feat_proj_dropout=0.0, final_dropout=0.0, layerdrop=0.0, mask_time_prob=0.0,
            mask_feature_prob=0.0)
FAMILIES = {"layer_preln": dict(feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True),
            "group_postln": dict(feat_extract_norm="group", do_stable_layer_norm=False, conv_bias=False)}


def _model(transformers, family, seed=0):
    torch.manual_seed(seed)
    m = transformers.Wav2Vec2Model(transformers.Wav2Vec2Config(**{**BASE, **FAMILIES[family]}))
    with torch.no_grad():                       # default init leaves the positional conv and LayerNorms near-trivial: make every parameter matter
        for n, p in m.named_parameters():
            if p.dim() == 1 and "bias" in n:
                p.add_(0.05 * torch.randn_like(p))
            elif "layer_norm.weight" in n:
                p.mul_(1.0 + 0.1 * torch.randn_like(p))
    return m


@pytest.mark.parametrize("family", list(FAMILIES))
def test_whole_model_matches_transformers_autograd_within_bf16_tolerance(family):
    transformers = pytest.importorskip("transformers")
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    ref = _model(transformers, family)
    ref.freeze_feature_encoder()
    ref.train()
    mine = _model(transformers, family)
    mine.load_state_dict(ref.state_dict())
    adapt = HuggingFaceEncoderAdapt(mine, mask_input=True, precision="fp32", train_precision="bf16").cuda().train()
    x = torch.randn(3, 4000, generator=torch.Generator().manual_seed(1))
    lengths = torch.tensor([4000, 3000, 2111])
    x = x * (torch.arange(x.shape[1])[None, :] < lengths[:, None])
    att = (torch.arange(x.shape[1])[None, :] < lengths[:, None]).long()
    out_ref = ref(x, attention_mask=att).last_hidden_state
    probe = torch.randn(out_ref.shape, generator=torch.Generator().manual_seed(5))
    (out_ref * probe).sum().backward()
    feats, _ = adapt(x.cuda(), lengths.cuda())
    got = feats.transpose(-1, -2)
    err = float((got.detach().cpu() - out_ref.detach()).abs().max())
    print(f"{family}: output max abs error {err:.3e} against scale {float(out_ref.detach().abs().max()):.3e}")
    assert err <= 3e-2 * max(1.0, float(out_ref.abs().max())), err
    assert err > 1e-6, "the mixed-precision path did not run"
    seen, todo = set(), [got.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        todo += [f for f, _ in fn.next_functions]
    names = {type(fn).__name__ for fn in seen}
    assert "AttentionFused80Backward" in names and "AttentionBackward" not in names and "AttentionFusedBackward" not in names, names
    (got * probe.cuda()).sum().backward()
    theirs = dict(adapt.original_encoder.named_parameters())
    # k_proj.bias has no true gradient (the softmax ignores a shift of a query's scores): both sides hold rounding noise there, so gradients are
    # measured against the larger of their own norm and 1e-4 of the model's largest gradient norm (as tests/test_gpu_w2v_train.py)
    floor = 1e-4 * max(float(p.grad.norm()) for p in ref.parameters() if p.grad is not None)
    checked = 0
    for name, p in ref.named_parameters():
        q = theirs[name]
        if not p.requires_grad:
            assert q.grad is None or float(q.grad.abs().max()) == 0.0, name
            continue
        assert p.grad is not None and q.grad is not None, name
        r = float((q.grad.cpu() - p.grad).norm()) / max(float(p.grad.norm()), floor)
        assert r <= 4e-2, (name, r)
        checked += 1
    assert checked > 20
    with torch.no_grad():
        feats2, _ = adapt(x.cuda(), lengths.cuda())
    assert torch.equal(feats2, feats)
