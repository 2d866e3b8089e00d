"""GPU parity of FINE-TUNING a rotary wav2vec2-conformer (thunder_speech_amd/huggingface/conformer_train.py on csrc/conformer_train.hip) against the
REAL transformers model in train mode with torch autograd on the CPU, built like tests/test_gpu_family_finetune.py (its batch, its floor rule for the
gradients, its perturbations -- plus batch_norm.weight): seeded random weights, hidden 128, 2 heads, intermediate 256, 2 layers, conv_dim (32, 32, 32),
strides (5, 2, 2), three ragged clips of 4000 / 3000 / 2111 samples (199 frames), all dropouts off unless a test says otherwise, the conv feature
extractor frozen.  The conformer trains in mixed precision only, so every comparison is at the project's mixed-precision bounds: last_hidden_state within
3e-2 x max(1, max |ref|), every parameter gradient within 4e-2 relative L2."""
import contextlib
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
transformers = pytest.importorskip("transformers")

from test_gpu_family_finetune import LENGTHS, _compare_grads, _graph_nodes, _inputs, _ragged       # noqa: E402  (the batch and the floor rule)

BASE = dict(vocab_size=32, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, conv_dim=(32, 32, 32),
            conv_stride=(5, 2, 2), conv_kernel=(10, 3, 2), num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=2, hidden_dropout=0.0,
            activation_dropout=0.0, attention_dropout=0.0, feat_proj_dropout=0.0, final_dropout=0.0, conformer_conv_dropout=0.0, layerdrop=0.0,
            mask_time_prob=0.0, mask_feature_prob=0.0, position_embeddings_type="rotary", hidden_act="swish", conv_depthwise_kernel_size=31)
VARIANTS = {"swish_k31": dict(hidden_act="swish", conv_depthwise_kernel_size=31), "gelu_k5": dict(hidden_act="gelu", conv_depthwise_kernel_size=5)}
OUT_TOL, GRAD_TOL = 3e-2, 4e-2


def _model(seed=0, head=False, **over):
    torch.manual_seed(seed)
    cfg = transformers.Wav2Vec2ConformerConfig(**{**BASE, **over})
    m = (transformers.Wav2Vec2ConformerForCTC if head else transformers.Wav2Vec2ConformerModel)(cfg)
    with torch.no_grad():                       # default init leaves LayerNorms and BatchNorms trivial: make every parameter matter
        for n, p in m.named_parameters():
            if p.dim() == 1 and "bias" in n:
                p.add_(0.05 * torch.randn_like(p))
            elif "layer_norm.weight" in n or "batch_norm.weight" in n:
                p.mul_(1.0 + 0.1 * torch.randn_like(p))
        base = m.base_model if head else m
        if getattr(base, "masked_spec_embed", None) is not None:
            base.masked_spec_embed.copy_(torch.randn_like(base.masked_spec_embed))
    return m


def _pair(seed=0, **over):
    """(reference model on the CPU, the same weights behind the HIP adapter on the GPU), both in train mode, feature extractor frozen."""
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    ref = _model(seed, **over)
    ref.freeze_feature_encoder()
    ref.train()
    mine = _model(seed, **over)
    mine.load_state_dict(ref.state_dict())
    adapt = HuggingFaceEncoderAdapt(mine, precision="fp32", train_precision="bf16").cuda().train()
    return ref, adapt


def _out_close(got, ref, what):
    err = float((got.detach().cpu() - ref.detach()).abs().max())
    bound = OUT_TOL * max(1.0, float(ref.abs().max()))
    print(f"{what}: output error {err:.4f} of {bound:.4f} allowed")
    assert err <= bound, (what, err, bound)
    return err


def _batch_norms(model):
    return [layer.conv_module.batch_norm for layer in model.encoder.layers]


# ---- what the fused attention's bf16 operands do to linear_k.bias: an emulation on the CPU ------------------------------------------------------
# linear_k.bias has NO true gradient (q . b_k is the same for every key of a row: the softmax does not see it); the reference's is float32 noise and
# the floor rule of _compare_grads measures this side's noise against 1e-4 of the model's largest gradient.  The fused backward forms
# dS = P (dP - D) with D = rowdot(dO, O) and O the product of bf16-ROUNDED probabilities (csrc/w2v_attn_train.hip), so a row of dS sums to the
# rounding error of that row instead of to zero, and the padded frames of a ragged batch -- equal rows in layer 0 -- add those errors up with one sign.
class _Bf16Matmul(torch.autograd.Function):
    """a @ b with both operands rounded to bf16 in all three products, float64 accumulation; a [..][k] activations, b a [k][n] weight view."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        r = lambda v: v.to(torch.bfloat16).double()
        return (r(a) @ r(b)).to(a.dtype)

    @staticmethod
    def backward(ctx, dy):
        a, b = ctx.saved_tensors
        r = lambda v: v.to(torch.bfloat16).double()
        da = r(dy) @ r(b).transpose(-1, -2)
        db = r(a).reshape(-1, a.shape[-1]).t() @ r(dy).reshape(-1, dy.shape[-1])
        return da.to(a.dtype), db.to(b.dtype)


class _FusedAttentionEmu(torch.autograd.Function):
    """The arithmetic the header of csrc/w2v_attn_train.hip states, head_dim 64: bf16 q, k, v, dO, P, dS; D from the f32 dO and O."""

    @staticmethod
    def forward(ctx, q, k, v, mask):
        r = lambda x: x.to(torch.bfloat16).double()
        s = r(q) @ r(k).transpose(-1, -2) / 8.0
        if mask is not None:
            s = s + mask.double()
        p = torch.softmax(s, -1)
        o = (r(p) @ r(v)).to(q.dtype)
        ctx.save_for_backward(q, k, v, p, o)
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, p, o = ctx.saved_tensors
        r = lambda x: x.to(torch.bfloat16).double()
        do16 = r(do)
        dv = r(p).transpose(-1, -2) @ do16
        dp = do16 @ r(v).transpose(-1, -2)
        d = (do.double() * o.double()).sum(-1, keepdim=True)
        ds = r(p * (dp - d))
        return (ds @ r(k) / 8.0).to(q.dtype), (ds.transpose(-1, -2) @ r(q) / 8.0).to(k.dtype), dv.to(v.dtype), None


def _attn_forward(att):
    def forward(hidden_states, attention_mask=None, relative_position_embeddings=None, output_attentions=False):
        b = hidden_states.shape[0]
        qk = att._apply_rotary_embedding(hidden_states, relative_position_embeddings)
        heads = lambda x: x.view(b, -1, att.num_heads, att.head_size).transpose(1, 2)
        o = _FusedAttentionEmu.apply(heads(att.linear_q(qk)), heads(att.linear_k(qk)), heads(att.linear_v(hidden_states)), attention_mask)
        return att.linear_out(o.transpose(1, 2).reshape(b, -1, att.num_heads * att.head_size)), None
    return forward


@contextlib.contextmanager
def _bf16_products(model):
    """Inside: every nn.Linear and 1 x 1 conv of the model multiplies bf16-rounded operands in its three products, and the attention core is
    _FusedAttentionEmu; everything else stays float32."""
    mods = [(layer.self_attn, _attn_forward(layer.self_attn)) for layer in model.encoder.layers]
    for m in model.modules():
        if isinstance(m, torch.nn.Linear):
            mods.append((m, (lambda m_: lambda x: _Bf16Matmul.apply(x, m_.weight.t()) + m_.bias)(m)))
        elif isinstance(m, torch.nn.Conv1d) and m.kernel_size == (1,) and m.groups == 1:
            mods.append((m, (lambda m_: lambda x: _Bf16Matmul.apply(x.transpose(1, 2), m_.weight.squeeze(-1).t()).transpose(1, 2))(m)))
    old = [m.forward for m, _ in mods]
    for m, f in mods:
        m.forward = f
    try:
        yield
    finally:
        for (m, _), f in zip(mods, old):
            m.forward = f


def _k_bias_bounds(ref, twin, x, att, probe):
    """{linear_k.bias of each layer: its bound}.  `ref`: the float32 reference after its backward; `twin`: the same model in the same state, run here under
    the emulation on the same batch.  Bound: twice the emulated error under the floor rule (twice, as in tests/test_gpu_family_finetune.py: the emulation has
    neither the kernels' f32 accumulation order nor their online softmax), and never below the 4e-2 every parameter has."""
    with _bf16_products(twin):
        out = twin(x, attention_mask=att).last_hidden_state
        (out * probe).sum().backward()
    want = {n: p.grad for n, p in ref.named_parameters() if p.grad is not None}
    floor = 1e-4 * max(float(g.norm()) for g in want.values())
    emulated = {n: float((p.grad - want[n]).norm()) / max(float(want[n].norm()), floor) for n, p in twin.named_parameters() if p.grad is not None}
    assert set(emulated) == set(want)
    others = [e for n, e in emulated.items() if not n.endswith("self_attn.linear_k.bias")]
    assert 5e-3 < max(others) < GRAD_TOL, max(others)                      # the emulation ran, rounded what it should, and stays inside the bound itself
    bounds = {n: max(GRAD_TOL, 2.0 * e) for n, e in emulated.items() if n.endswith("self_attn.linear_k.bias")}
    print("emulated linear_k.bias errors", {n: round(e, 4) for n, e in emulated.items() if n in bounds}, "worst other parameter", round(max(others), 4))
    return bounds


def _reference(seed=0, **over):
    m = _model(seed, **over)
    m.freeze_feature_encoder()
    return m.train()


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_mixed_precision_training_matches_transformers_autograd(variant, masked):
    """last_hidden_state and the gradient of EVERY trainable parameter of a scalar loss, with and without an attention mask.  The positional conv's
    parameters have no gradient on either side (_compare_grads); the graph holds the conformer's own nodes and the fused attention; the forward
    is bit-reproducible.

    Every parameter holds 4e-2 but linear_k.bias of layer 0 on the ragged batch, which has no true gradient (block above): measured on an MI355X 0.162
    (swish, k 31) and 0.154 (gelu, k 5) against 0.178 and 0.134 from the CPU emulation of the fused attention's arithmetic, i.e. allowed 0.355 and 0.269;
    without a mask 0.0196 and 0.0178 (emulated 0.0211, 0.0234).  The worst parameter WITH a true gradient: measured 0.015, emulated 0.016.  The emulated
    output error is 0.027 - 0.037 of the 0.15 - 0.16 allowed, measured 0.028 - 0.033."""
    ref, adapt = _pair(**VARIANTS[variant])
    adapt.mask_input = masked
    x, att = _ragged(masked)
    out_ref = ref(x, attention_mask=att).last_hidden_state
    probe = torch.randn(out_ref.shape, generator=torch.Generator().manual_seed(5))
    (out_ref * probe).sum().backward()
    feats, _ = adapt(x.cuda(), LENGTHS.cuda())
    assert feats.shape == (3, out_ref.shape[2], out_ref.shape[1]) and out_ref.shape[1] == 199
    got = feats.transpose(-1, -2)
    err = _out_close(got, out_ref, f"{variant} masked={masked}")
    assert err > 1e-6, "the mixed-precision path did not run (bit-level agreement with f32 is not what bf16 operands give)"
    names = _graph_nodes(got)
    for node in ("AttentionFusedBackward", "LayerNormRotaryBackward", "RotaryQKVBackward", "GluDwconvBnActBackward", "FFNActLinearBackward",
                 "LinearMixedBackward"):
        assert node in names, (node, names)
    (got * probe.cuda()).sum().backward()
    k_bias = _k_bias_bounds(ref, _reference(**VARIANTS[variant]), x, att, probe)
    errs = _compare_grads(ref, adapt, tol=GRAD_TOL, tol_of=k_bias.get)
    worst = max(errs, key=errs.get)
    with_gradient = max(e for n, e in errs.items() if n not in k_bias)
    print(variant, masked, "worst gradient error", worst, errs[worst], "worst parameter with a true gradient", with_gradient)
    assert max(errs.values()) > 1e-5
    for n, p in adapt.original_encoder.named_parameters():
        if "pos_conv_embed" in n:
            assert p.grad is None, n
    bn_names = [n for n in errs if "batch_norm" in n or "depthwise_conv" in n or "pointwise_conv" in n]
    assert len(bn_names) == 2 * 5, bn_names
    before = [(bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked)) for bn in _batch_norms(adapt.original_encoder)]
    with torch.no_grad():
        feats2, _ = adapt(x.cuda(), LENGTHS.cuda())
    assert torch.equal(feats2, feats)
    for bn, (m0, v0, n0) in zip(_batch_norms(adapt.original_encoder), before):
        assert int(bn.num_batches_tracked) == n0 + 1 and not torch.equal(bn.running_mean, m0) and not torch.equal(bn.running_var, v0)


def test_batchnorm_buffers_follow_transformers_after_one_training_forward():
    ref, adapt = _pair()
    adapt.mask_input = True
    x, att = _ragged(True)
    ref(x, attention_mask=att)
    with torch.no_grad():
        adapt(x.cuda(), LENGTHS.cuda())
    for i, (a, b) in enumerate(zip(_batch_norms(ref), _batch_norms(adapt.original_encoder))):
        assert int(b.num_batches_tracked) == int(a.num_batches_tracked) == 1
        for name in ("running_mean", "running_var"):
            want, got = getattr(a, name), getattr(b, name).cpu()
            err, scale = float((got - want).abs().max()), float(want.abs().max())
            print(f"layer {i} {name}: error {err:.3e} of {OUT_TOL * scale:.3e} allowed")
            assert err <= OUT_TOL * scale, (i, name, err, scale)
            assert not torch.equal(got, torch.zeros_like(got)) and not torch.equal(got, torch.ones_like(got))


def test_a_batchnorm_in_eval_mode_uses_and_keeps_its_running_statistics():
    """Every batch_norm in .eval() on both sides, inside training encoders, with running statistics that are not the initial (0, 1): buffers unchanged,
    output and gradients at the same bounds."""
    ref, adapt = _pair(seed=2)
    twin = _reference(seed=2)
    g = torch.Generator().manual_seed(9)
    for a, b, c in zip(_batch_norms(ref), _batch_norms(adapt.original_encoder), _batch_norms(twin)):
        rm, rv = 0.05 * torch.randn(128, generator=g), 0.02 + 0.05 * torch.rand(128, generator=g)
        for bn in (a, b, c):
            with torch.no_grad():
                bn.running_mean.copy_(rm)
                bn.running_var.copy_(rv)
            bn.eval()
    adapt.mask_input = True
    x, att = _ragged(True)
    out_ref = ref(x, attention_mask=att).last_hidden_state
    probe = torch.randn(out_ref.shape, generator=torch.Generator().manual_seed(5))
    (out_ref * probe).sum().backward()
    kept = [(bn.running_mean.clone(), bn.running_var.clone()) for bn in _batch_norms(adapt.original_encoder)]
    feats, _ = adapt(x.cuda(), LENGTHS.cuda())
    got = feats.transpose(-1, -2)
    _out_close(got, out_ref, "batch_norm.eval()")
    (got * probe.cuda()).sum().backward()
    # linear_k.bias of layer 0 (no true gradient): measured 0.042, emulated 0.068
    errs = _compare_grads(ref, adapt, tol=GRAD_TOL, tol_of=_k_bias_bounds(ref, twin, x, att, probe).get)
    print("batch_norm.eval(): worst gradient error", max(errs.values()))
    for bn, (m0, v0) in zip(_batch_norms(adapt.original_encoder), kept):
        assert torch.equal(bn.running_mean, m0) and torch.equal(bn.running_var, v0) and int(bn.num_batches_tracked) == 0


def test_eval_after_a_training_forward_without_an_optimizer_step_uses_the_new_running_statistics():
    """The inference plan folds running_mean / running_var into its BatchNorm scale and shift.  A train-mode forward changes those buffers and no
    parameter: eval() afterwards must give what a fresh adapter built from the same state dict gives, not the plan packed before."""
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    _, adapt = _pair(seed=4)
    adapt.mask_input = True
    x = _ragged(True)[0].cuda()
    adapt.eval()
    with torch.no_grad():
        stale, _ = adapt(x, LENGTHS.cuda())                 # packs the plan on the initial statistics
    adapt.train()
    with torch.no_grad():
        adapt(x, LENGTHS.cuda())
    adapt.eval()
    with torch.no_grad():
        got, _ = adapt(x, LENGTHS.cuda())
    fresh_model = _model(seed=4)
    fresh_model.load_state_dict(adapt.original_encoder.state_dict())
    fresh = HuggingFaceEncoderAdapt(fresh_model, mask_input=True, precision="fp32").cuda().eval()
    with torch.no_grad():
        want, _ = fresh(x, LENGTHS.cuda())
    assert torch.equal(got, want)
    assert not torch.equal(got, stale)


def test_time_masking_follows_transformers_under_the_same_numpy_seed():
    ref, adapt = _pair(mask_time_prob=0.3, mask_time_length=3, mask_time_min_masks=2)
    x = _inputs(b=2, n=6000, seed=2)
    np.random.seed(11)
    out_ref = ref(x).last_hidden_state
    probe = torch.randn(out_ref.shape, generator=torch.Generator().manual_seed(6))
    (out_ref * probe).sum().backward()
    np.random.seed(11)
    feats, _ = adapt(x.cuda(), torch.tensor([6000, 6000]).cuda())
    got = feats.transpose(-1, -2)
    _out_close(got, out_ref, "time masking")
    (got * probe.cuda()).sum().backward()
    _compare_grads(ref, adapt, tol=GRAD_TOL)
    assert float(adapt.original_encoder.masked_spec_embed.grad.abs().max()) > 0


def test_layerdrop_skips_the_same_layers_as_transformers_under_the_same_torch_seed():
    ref, adapt = _pair(layerdrop=0.5, num_hidden_layers=4)
    x = _inputs(b=2, n=3000, seed=3)
    torch.manual_seed(21)
    draws = [float(torch.rand([])) < 0.5 for _ in range(4)]
    assert any(draws) and not all(draws)                    # the seed skips some layers and runs others
    torch.manual_seed(21)
    out_ref = ref(x).last_hidden_state
    torch.manual_seed(21)
    feats, _ = adapt(x.cuda(), torch.tensor([3000, 3000]).cuda())
    _out_close(feats.transpose(-1, -2), out_ref, "layerdrop")
    tracked = [int(bn.num_batches_tracked) for bn in _batch_norms(adapt.original_encoder)]
    assert tracked == [int(bn.num_batches_tracked) for bn in _batch_norms(ref)] == [0 if d else 1 for d in draws]


def test_with_every_dropout_on_two_forwards_differ_and_the_backward_is_finite():
    _, adapt = _pair(hidden_dropout=0.1, activation_dropout=0.1, attention_dropout=0.1, feat_proj_dropout=0.1, final_dropout=0.1,
                     conformer_conv_dropout=0.1)
    adapt.mask_input = True
    x = _ragged(True)[0].cuda()
    torch.manual_seed(1)
    a, _ = adapt(x, LENGTHS.cuda())
    b, _ = adapt(x, LENGTHS.cuda())
    assert not torch.equal(a, b)
    for out in (a, b):
        assert bool(torch.isfinite(out).all()) and 0.5 < float(out.std()) < 2.0          # behind the encoder's LayerNorm: unit scale
    a.square().mean().backward()
    n = 0
    for name, p in adapt.original_encoder.named_parameters():
        if p.requires_grad and "pos_conv_embed" not in name and name != "masked_spec_embed":
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
            n += 1
    assert n > 60


def test_fp32_training_is_still_refused_by_name_on_the_gpu():
    _, adapt = _pair()
    adapt.train_precision = "fp32"
    with pytest.raises(NotImplementedError, match="wav2vec2-conformer"):
        adapt(_inputs().cuda(), LENGTHS.cuda())


def test_a_batch_of_one_frame_raises_as_torch_does_before_any_launch():
    """B = 1 and 40 samples are one frame: BatchNorm in training has one value per channel.  transformers raises torch's ValueError; so does this side."""
    ref, adapt = _pair()
    x = _inputs(b=1, n=40, seed=4)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        ref(x)
    from thunder_speech_amd import _lib
    calls = _lib.CALLS
    with pytest.raises(ValueError, match=r"Expected more than 1 value per channel when training, got input size torch.Size\(\[1, 128, 1\]\)"):
        adapt(x.cuda(), torch.tensor([40]).cuda())
    assert _lib.CALLS == calls


def test_five_training_steps_through_the_module_lower_the_loss_and_predict_runs_afterwards(tmp_path):
    """module_from_huggingface(Wav2Vec2ConformerForCTC) in mixed precision: five training_step + optimizer steps on one fixed batch; the loss is finite
    and lower at step 5; predict() afterwards runs on the updated weights and the updated running statistics (the plan is re-packed)."""
    from thunder_speech_amd.huggingface.compatibility import module_from_huggingface
    tokens = ["<pad>", "<s>", "</s>", "<unk>", "|"] + [chr(97 + i) for i in range(26)] + ["'"]
    vocab = tmp_path / "vocab.json"
    vocab.write_text(json.dumps({tok: i for i, tok in enumerate(tokens)}))
    tokenizer = transformers.Wav2Vec2CTCTokenizer(str(vocab))
    model = _model(seed=3, head=True, vocab_size=len(tokens), pad_token_id=0)
    module = module_from_huggingface(model, transformers.Wav2Vec2FeatureExtractor(return_attention_mask=True), tokenizer)
    module.encoder.train_precision = "bf16"
    module.optimizer_kwargs = {"lr": 1e-3}
    batch = (_inputs(b=2, n=8000, seed=7).cuda(), torch.tensor([8000.0, 6000.0]).cuda(), ["hello world", "abc"])
    module = module.cuda().eval()
    with torch.no_grad():
        before, _ = module.encoder(batch[0], batch[1])
    module.train()
    opt = module.configure_optimizers()
    opt = opt["optimizer"] if isinstance(opt, dict) else opt
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = module.training_step(batch, 0)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print("conformer", losses)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    bns = _batch_norms(module.encoder.original_encoder)
    assert all(int(bn.num_batches_tracked) == 5 for bn in bns)
    module.eval()
    with torch.no_grad():
        after, _ = module.encoder(batch[0], batch[1])
    assert bool(torch.isfinite(after).all()) and not torch.equal(after, before)
    text = module.predict(batch[0][:1])
    assert isinstance(text, list) and len(text) == 1 and isinstance(text[0], str)
