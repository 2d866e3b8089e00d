"""GPU parity of FINE-TUNING a SEW encoder (thunder_speech_amd/huggingface/sew_train.py on csrc/sew_train.hip) against the REAL transformers SEWModel in
train mode with torch autograd on the CPU, built like tests/test_gpu_conformer_train.py (the batch, the floor rule for the gradients and the
perturbations of tests/test_gpu_family_finetune.py): seeded random weights, hidden 128, 2 heads, intermediate 256, 2 layers, 4 groups of 32 channels,
16 taps, squeeze_factor 2, conv_dim (32, 32, 64) so that the feature projection exists, strides (5, 2, 2), three ragged clips of 4000 / 3000 / 2111
samples (199 frames: T % 2 = 1), all dropouts off unless a test says otherwise, the conv feature extractor frozen.  SEW trains in mixed precision only,
so every comparison is at the project's mixed-precision bounds: last_hidden_state within 3e-2 x max(1, max |ref|), every parameter gradient within 4e-2
relative L2 under the floor rule; k_proj.bias (no true gradient) is held to twice a CPU emulation of the fused attention, never below 4e-2."""
import contextlib
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
transformers = pytest.importorskip("transformers")

from test_gpu_conformer_train import _Bf16Matmul, _FusedAttentionEmu                               # noqa: E402  (the emulated bf16 products)
from test_gpu_family_finetune import _compare_grads, _graph_nodes, _inputs                          # noqa: E402  (the batch and the floor rule)

BASE = dict(vocab_size=32, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, conv_dim=(32, 32, 64),
            conv_stride=(5, 2, 2), conv_kernel=(10, 3, 2), num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, squeeze_factor=2,
            hidden_dropout=0.0, activation_dropout=0.0, attention_dropout=0.0, feat_proj_dropout=0.0, final_dropout=0.0, layerdrop=0.0,
            mask_time_prob=0.0, mask_feature_prob=0.0)
# (configuration, samples of the longest clip): 4000 samples are 199 frames, 4010 are 200
VARIANTS = {"s2_odd": (dict(), 4000),                                                               # T % 2 = 1: the padding node
            "cg24_k15": (dict(hidden_size=192, num_attention_heads=3, num_conv_pos_embedding_groups=8, num_conv_pos_embeddings=15), 4000),
            "s3": (dict(squeeze_factor=3), 4010),                                                   # T % 3 = 2
            "s2_even": (dict(), 4010),                                                              # no padding node
            "no_projection": (dict(conv_dim=(32, 32, 128)), 4000)}
OUT_TOL, GRAD_TOL = 3e-2, 4e-2
ATEN_ON_ACTIVATIONS = ("ConvolutionBackward0", "MmBackward0", "AddmmBackward0", "BmmBackward0", "NativeLayerNormBackward0", "GeluBackward0",
                       "SoftmaxBackward0", "AvgPool2DBackward0", "NativeDropoutBackward0")


def _model(seed=0, head=False, **over):
    torch.manual_seed(seed)
    cfg = transformers.SEWConfig(**{**BASE, **over})
    m = (transformers.SEWForCTC if head else transformers.SEWModel)(cfg)
    with torch.no_grad():                       # default init leaves biases zero and LayerNorms trivial: make every parameter matter
        for n, p in m.named_parameters():
            if p.dim() == 1 and "bias" in n:
                p.add_(0.05 * torch.randn_like(p))
            elif "layer_norm.weight" in n:
                p.mul_(1.0 + 0.1 * torch.randn_like(p))
        base = m.base_model if head else m
        if getattr(base, "masked_spec_embed", None) is not None:
            base.masked_spec_embed.copy_(torch.randn_like(base.masked_spec_embed))
    return m


def _reference(seed=0, **over):
    m = _model(seed, **over)
    m.feature_extractor._freeze_parameters()                # SEWModel has no freeze_feature_encoder (only its ForCTC wrapper does)
    return m.train()


def _pair(seed=0, **over):
    """(reference model on the CPU, the same weights behind the HIP adapter on the GPU), both in train mode, feature extractor frozen."""
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    ref = _reference(seed, **over)
    mine = _model(seed, **over)
    mine.load_state_dict(ref.state_dict())
    adapt = HuggingFaceEncoderAdapt(mine, precision="fp32", train_precision="bf16").cuda().train()
    return ref, adapt


def _batch(n, masked):
    """three clips of n / 3000 / 2111 samples -> (audio, transformers' attention mask or None, lengths)"""
    lengths = torch.tensor([n, 3000, 2111])
    x = _inputs(n=n)
    if not masked:
        return x, None, lengths
    keep = torch.arange(n)[None, :] < lengths[:, None]
    return x * keep, keep.long(), lengths


def _out_close(got, ref, what):
    err = float((got.detach().cpu() - ref.detach()).abs().max())
    bound = OUT_TOL * max(1.0, float(ref.abs().max()))
    print(f"{what}: output error {err:.4f} of {bound:.4f} allowed (max |ref| {float(ref.abs().max()):.3f})")
    assert err <= bound, (what, err, bound)
    return err


# ---- what the bf16 operands do to k_proj.bias: the emulation of tests/test_gpu_conformer_train.py on SEW's modules --------------------------------
class _Bf16Conv(torch.autograd.Function):
    """grouped strided conv1d with both operands rounded to bf16 in all three products, float64 accumulation"""

    @staticmethod
    def forward(ctx, x, w, stride, padding, groups):
        ctx.save_for_backward(x, w)
        ctx.geom = (stride, padding, groups)
        r = lambda v: v.to(torch.bfloat16).double()
        return F.conv1d(r(x), r(w), None, stride, padding, 1, groups).to(x.dtype)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        stride, padding, groups = ctx.geom
        r = lambda v: v.to(torch.bfloat16).double()
        dx = torch.nn.grad.conv1d_input(x.shape, r(w), r(dy), stride, padding, 1, groups)
        dw = torch.nn.grad.conv1d_weight(r(x), w.shape, r(dy), stride, padding, 1, groups)
        return dx.to(x.dtype), dw.to(w.dtype), None, None, None


def _attn_forward(att):
    def forward(hidden_states, key_value_states=None, attention_mask=None, output_attentions=False, **kw):
        b = hidden_states.shape[0]
        heads = lambda x: x.view(b, -1, att.num_heads, att.head_dim).transpose(1, 2)
        o = _FusedAttentionEmu.apply(heads(att.q_proj(hidden_states)), heads(att.k_proj(hidden_states)), heads(att.v_proj(hidden_states)), attention_mask)
        return att.out_proj(o.transpose(1, 2).reshape(b, -1, att.num_heads * att.head_dim)), None, None
    return forward


@contextlib.contextmanager
def _bf16_products(model):
    """Inside: every nn.Linear and the strided positional conv multiply bf16-rounded operands in their three products and the attention core is
    _FusedAttentionEmu; everything else stays float32."""
    mods = [(layer.attention, _attn_forward(layer.attention)) for layer in model.encoder.layers]
    for m in model.modules():
        if isinstance(m, torch.nn.Linear):
            mods.append((m, (lambda m_: lambda x: _Bf16Matmul.apply(x, m_.weight.t()) + m_.bias)(m)))
    conv = model.encoder.pos_conv_embed.conv
    mods.append((conv, lambda x: _Bf16Conv.apply(x, conv.weight, conv.stride[0], conv.padding[0], conv.groups) + conv.bias[None, :, None]))
    old = [m.forward for m, _ in mods]
    for m, f in mods:
        m.forward = f
    try:
        yield
    finally:
        for (m, _), f in zip(mods, old):
            m.forward = f


def _k_bias_bounds(ref, twin, x, att, probe):
    """{k_proj.bias of each layer: its bound}: twice the error of the emulation under the floor rule, never below the 4e-2 every parameter has (the rule
    and the reasons of tests/test_gpu_conformer_train.py::_k_bias_bounds).  `ref`: the float32 reference after its backward; `twin`: the same model in
    the same state, run here under the emulation on the same batch."""
    with _bf16_products(twin):
        out = twin(x, attention_mask=att).last_hidden_state
        (out * probe).sum().backward()
    want = {n: p.grad for n, p in ref.named_parameters() if p.grad is not None}
    floor = 1e-4 * max(float(g.norm()) for g in want.values())
    emulated = {n: float((p.grad - want[n]).norm()) / max(float(want[n].norm()), floor) for n, p in twin.named_parameters() if p.grad is not None}
    assert set(emulated) == set(want)
    others = [e for n, e in emulated.items() if not n.endswith("attention.k_proj.bias")]
    assert 1e-3 < max(others) < GRAD_TOL, max(others)                      # the emulation ran, rounded what it should, and stays inside the bound itself
    bounds = {n: max(GRAD_TOL, 2.0 * e) for n, e in emulated.items() if n.endswith("attention.k_proj.bias")}
    print("emulated k_proj.bias errors", {n: round(e, 4) for n, e in emulated.items() if n in bounds}, "worst other parameter", round(max(others), 4))
    return bounds


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_mixed_precision_training_matches_transformers_autograd(variant, masked):
    """last_hidden_state and the gradient of EVERY trainable parameter of a scalar loss, with and without an attention mask -- the positional conv's
    g / v / bias, the upsampling projection, the model-level layer_norm and the feature projection among them; the graph holds this library's nodes and
    no ATen conv / matmul node on an activation; the forward is bit-reproducible.

    Measured on an MI355X over the ten cases: output error 0.0024 - 0.0036 against 0.030 - 0.033 allowed; worst gradient 0.0100 - 0.0142, always a q / k
    projection weight (the CPU emulation of the bf16 products gives 0.0100 - 0.0123 for its worst parameter); k_proj.bias inside 4e-2 everywhere
    (emulated 0.0017 - 0.0053: SEW zeroes the padded frames BEFORE the squeeze, the rows the attention sees are not equal)."""
    over, n = VARIANTS[variant]
    ref, adapt = _pair(**over)
    adapt.mask_input = masked
    x, att, lengths = _batch(n, masked)
    out_ref = ref(x, attention_mask=att).last_hidden_state
    probe = torch.randn(out_ref.shape, generator=torch.Generator().manual_seed(5))
    (out_ref * probe).sum().backward()
    feats, _ = adapt(x.cuda(), lengths.cuda())
    t, s = out_ref.shape[1], ref.config.squeeze_factor
    assert feats.shape == (3, out_ref.shape[2], t) and t == (199 if n == 4000 else 200)
    got = feats.transpose(-1, -2)
    err = _out_close(got, out_ref, f"{variant} masked={masked}")
    assert err > 1e-6, "the mixed-precision path did not run (bit-level agreement with f32 is not what bf16 operands give)"
    if t % s:
        assert not bool(got[:, s * (t // s):].any()) and not bool(out_ref[:, s * (t // s):].any())
    names = _graph_nodes(got)
    for node in ("SqueezeGeluBackward", "AttentionFusedBackward", "FFNActLinearBackward", "LinearMixedBackward", "BiasGeluBackward", "LayerNormBackward"):
        assert node in names, (node, names)
    assert ("UnsqueezeRowsBackward" in names) is (t % s != 0), names
    assert ("MaskRowsBackward" in names) is masked
    assert not names & set(ATEN_ON_ACTIVATIONS), names & set(ATEN_ON_ACTIVATIONS)
    (got * probe.cuda()).sum().backward()
    k_bias = _k_bias_bounds(ref, _reference(**over), x, att, probe)
    errs = _compare_grads(ref, adapt, tol=GRAD_TOL, tol_of=k_bias.get)
    worst = max(errs, key=errs.get)
    print(variant, masked, "worst gradient error", worst, errs[worst], "worst parameter with a true gradient", max(e for n, e in errs.items() if n not in k_bias))
    assert max(errs.values()) > 1e-5
    must = ["encoder.pos_conv_embed.conv.bias", "encoder.pos_conv_embed.conv.parametrizations.weight.original0",
            "encoder.pos_conv_embed.conv.parametrizations.weight.original1", "encoder.upsample.projection.weight", "encoder.upsample.projection.bias",
            "layer_norm.weight", "layer_norm.bias", "encoder.layer_norm.weight"]
    if variant != "no_projection":
        must += ["feature_projection.weight", "feature_projection.bias"]
    for name in must:
        assert name in errs, (name, sorted(errs))
        print(f"  {name}: {errs[name]:.4f}")
    assert ("feature_projection.weight" in errs) is (variant != "no_projection")
    with torch.no_grad():
        feats2, _ = adapt(x.cuda(), lengths.cuda())
    assert torch.equal(feats2, feats)


class _seeded_twin:
    """A reference twin whose forward re-seeds numpy first, so that the emulation draws the spans the reference drew."""

    def __init__(self, seed, **over):
        self.model, self.seed = _reference(**over), seed

    def __call__(self, *a, **kw):
        np.random.seed(self.seed)
        return self.model(*a, **kw)

    def __getattr__(self, name):
        return getattr(self.model, name)


def test_time_masking_follows_transformers_under_the_same_numpy_seed():
    """SEWModel draws its spans WITHOUT the attention mask: under the same numpy seed the same frames are masked on both sides, padded frames included."""
    from thunder_speech_amd.huggingface import train as T
    over = dict(mask_time_prob=0.3, mask_time_length=3, mask_time_min_masks=2)
    ref, adapt = _pair(**over)
    adapt.mask_input = True
    x, att, lengths = _batch(4000, True)
    np.random.seed(11)
    drawn = T.compute_mask_indices(3, 199, 0.3, 3, None, 2)
    assert drawn[2, 110:].any(), "no span on the padded frames of the shortest clip (105 valid frames): the case shows nothing"
    np.random.seed(11)
    out_ref = ref(x, attention_mask=att).last_hidden_state
    probe = torch.randn(out_ref.shape, generator=torch.Generator().manual_seed(6))
    (out_ref * probe).sum().backward()
    np.random.seed(11)
    feats, _ = adapt(x.cuda(), lengths.cuda())
    got = feats.transpose(-1, -2)
    _out_close(got, out_ref, "time masking")
    assert "MaskEmbedBackward" in _graph_nodes(got)
    (got * probe.cuda()).sum().backward()
    k_bias = _k_bias_bounds(ref, _seeded_twin(11, **over), x, att, probe)
    errs = _compare_grads(ref, adapt, tol=GRAD_TOL, tol_of=k_bias.get)
    assert "masked_spec_embed" in errs and float(adapt.original_encoder.masked_spec_embed.grad.abs().max()) > 0
    print("masked_spec_embed gradient error", errs["masked_spec_embed"])


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
    got = feats.transpose(-1, -2)
    _out_close(got, out_ref, "layerdrop")
    (got * got).sum().backward()
    for i, layer in enumerate(adapt.original_encoder.encoder.layers):
        assert (layer.feed_forward.output_dense.weight.grad is None) is draws[i], (i, draws)


def test_with_every_dropout_on_two_forwards_differ_and_the_backward_is_finite():
    _, adapt = _pair(hidden_dropout=0.1, activation_dropout=0.1, attention_dropout=0.1, feat_proj_dropout=0.1, final_dropout=0.1)
    adapt.mask_input = True
    x, _, lengths = _batch(4000, True)
    torch.manual_seed(1)
    a, _ = adapt(x.cuda(), lengths.cuda())
    b, _ = adapt(x.cuda(), lengths.cuda())
    assert not torch.equal(a, b) and bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
    a.square().mean().backward()
    n = 0
    for name, p in adapt.original_encoder.named_parameters():
        if p.requires_grad and name != "masked_spec_embed":
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
            n += 1
    assert n > 40


def test_fp32_training_is_still_refused_by_name_on_the_gpu():
    _, adapt = _pair()
    adapt.train_precision = "fp32"
    with pytest.raises(NotImplementedError, match="sew: fine-tuning is not implemented"):
        adapt(_inputs().cuda(), torch.tensor([4000, 3000, 2111]).cuda())


def test_five_training_steps_through_the_module_lower_the_loss_and_eval_follows_the_updated_weights(tmp_path):
    """module_from_huggingface(SEWForCTC) with train_precision="bf16": five training_step + optimizer steps on one fixed batch; the loss is finite and
    lower at step 5; predict() afterwards runs on the updated weights; back in eval() the inference plan gives what transformers gives for the updated
    weights, within the f32 bound of tests/test_gpu_sew.py (atol 5e-4, rtol 1e-4)."""
    from thunder_speech_amd.huggingface.compatibility import module_from_huggingface
    tokens = ["<pad>", "<s>", "</s>", "<unk>", "|"] + [chr(97 + i) for i in range(26)] + ["'"]
    vocab = tmp_path / "vocab.json"
    vocab.write_text(json.dumps({tok: i for i, tok in enumerate(tokens)}))
    tokenizer = transformers.Wav2Vec2CTCTokenizer(str(vocab))
    model = _model(seed=3, head=True, vocab_size=len(tokens), pad_token_id=0)
    module = module_from_huggingface(model, transformers.Wav2Vec2FeatureExtractor(return_attention_mask=True), tokenizer)
    module.encoder.train_precision = "bf16"
    module.encoder.precision = "fp32"
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
    print("sew", losses)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    module.eval()
    with torch.no_grad():
        after, out_len = module.encoder(batch[0], batch[1])
    assert bool(torch.isfinite(after).all()) and not torch.equal(after, before)
    text = module.predict(batch[0][:1])
    assert isinstance(text, list) and len(text) == 1 and isinstance(text[0], str)
    fresh = _model(seed=3, head=True, vocab_size=len(tokens), pad_token_id=0).eval()
    fresh.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    mask = (torch.arange(8000)[None, :] < torch.tensor([8000, 6000])[:, None]).long()
    with torch.no_grad():
        want = fresh.base_model(batch[0].cpu(), attention_mask=mask).last_hidden_state
    got = after.transpose(1, 2).cpu()
    for i, n_i in enumerate(out_len.tolist()):
        np.testing.assert_allclose(got[i, :int(n_i)].numpy(), want[i, :int(n_i)].numpy(), atol=5e-4, rtol=1e-4)
