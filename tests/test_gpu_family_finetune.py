"""GPU parity of FINE-TUNING HuBERT, UniSpeech, UniSpeech-SAT and data2vec-audio (thunder_speech_amd/huggingface/train.py; data2vec's positional
stack on csrc/posconv_stack_train.hip) against the REAL transformers models in train mode with torch autograd on the CPU, built like
tests/test_gpu_w2v_train.py: seeded random weights, every bias perturbed (with transformers' zero conv biases the zeroed padded rows of a ragged batch
have variance exactly 0 in layer 1 of data2vec's stack and the reference's own bias gradient is meaningless), all dropouts off, the conv feature
extractor frozen.  The bounds are the ones that file holds wav2vec2 to: f32 mode 5e-4 / 3e-3, mixed precision 3e-2 / 4e-2."""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
transformers = pytest.importorskip("transformers")

BASE = dict(vocab_size=32, hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128, conv_dim=(32, 32, 32),
            conv_stride=(5, 2, 2), conv_kernel=(10, 3, 2), num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, hidden_dropout=0.0,
            activation_dropout=0.0, attention_dropout=0.0, feat_proj_dropout=0.0, final_dropout=0.0, layerdrop=0.0, mask_time_prob=0.0,
            mask_feature_prob=0.0)
# head_dim 64 and 64 channels per positional-conv group: mixed precision takes the fused attention and the matrix-core positional convs
HD64 = dict(hidden_size=128, num_attention_heads=2, intermediate_size=256, num_conv_pos_embedding_groups=2)
D2V = dict(num_conv_pos_embeddings=3, conv_pos_kernel_size=19)
FAMILIES = {
    "hubert": ("Hubert", dict(feat_proj_layer_norm=False, feat_extract_norm="group", do_stable_layer_norm=False, conv_bias=False)),
    "hubert_large": ("Hubert", dict(feat_proj_layer_norm=True, feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True)),
    "hubert_hd64": ("Hubert", dict(feat_proj_layer_norm=False, feat_extract_norm="group", do_stable_layer_norm=False, conv_bias=False, **HD64)),
    "unispeech": ("UniSpeech", dict(feat_extract_norm="group", do_stable_layer_norm=False, conv_bias=False)),
    "unispeech_sat": ("UniSpeechSat", dict(feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True)),
    "data2vec_k19": ("Data2VecAudio", dict(D2V)),
    "data2vec_k8": ("Data2VecAudio", dict(D2V, conv_pos_kernel_size=8)),
    "data2vec_k19_hd64": ("Data2VecAudio", dict(D2V, **HD64)),
    "data2vec_k8_hd64": ("Data2VecAudio", dict(D2V, conv_pos_kernel_size=8, **HD64)),
}
LENGTHS = torch.tensor([4000, 3000, 2111])


def _config(family, **over):
    cls, kw = FAMILIES[family]
    return getattr(transformers, cls + "Config")(**{**BASE, **kw, **over})


def _model(family, seed=0, head=False, **over):
    torch.manual_seed(seed)
    cls = FAMILIES[family][0]
    m = getattr(transformers, cls + ("ForCTC" if head else "Model"))(_config(family, **over))
    with torch.no_grad():                       # default init leaves the positional convs and LayerNorms near-trivial: make every parameter matter
        for n, p in m.named_parameters():
            if p.dim() == 1 and "bias" in n:
                p.add_(0.05 * torch.randn_like(p))
            elif "layer_norm.weight" in n:
                p.mul_(1.0 + 0.1 * torch.randn_like(p))
        base = m.base_model if head else m
        if getattr(base, "masked_spec_embed", None) is not None:
            base.masked_spec_embed.copy_(torch.randn_like(base.masked_spec_embed))
    return m


def _pair(family, seed=0, **over):
    """(reference model on the CPU, the same weights behind the HIP adapter on the GPU), both in train mode, feature extractor frozen."""
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    ref = _model(family, seed, **over)
    ref.feature_extractor._freeze_parameters()          # HubertModel has no freeze_feature_encoder
    ref.train()
    mine = _model(family, seed, **over)
    mine.load_state_dict(ref.state_dict())
    mine.feature_extractor._freeze_parameters()
    adapt = HuggingFaceEncoderAdapt(mine, precision="fp32").cuda().train()
    return ref, adapt


def _inputs(b=3, n=4000, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(b, n, generator=g)


def _compare_grads(ref, adapt, tol=3e-3, tol_of=None):
    """The floor rule of tests/test_gpu_w2v_train.py (k_proj.bias has no true gradient: errors are measured against the larger of a gradient's own norm and
    1e-4 of the model's largest), for models that also hold parameters OUTSIDE the forward (UniSpeech-SAT's speaker heads, the pre-training quantisers): where
    the reference has no gradient there is none here.  `tol_of(name)` may give a parameter its own bound.  -> {name: relative L2 error}"""
    mine = dict(adapt.original_encoder.named_parameters())
    floor = 1e-4 * max(float(p.grad.norm()) for p in ref.parameters() if p.grad is not None)
    errs = {}
    for name, p in ref.named_parameters():
        q = mine[name]
        if not p.requires_grad:
            assert q.grad is None or float(q.grad.abs().max()) == 0.0, name        # frozen feature extractor: no gradient
            continue
        if p.grad is None:
            assert q.grad is None, f"{name}: a gradient here, none in the reference"
            continue
        assert q.grad is not None, name
        assert bool(torch.isfinite(q.grad).all()), name
        errs[name] = float((q.grad.cpu() - p.grad).norm()) / max(float(p.grad.norm()), floor)
        bound = tol_of(name) if tol_of is not None and tol_of(name) is not None else tol
        assert errs[name] <= bound, (name, errs[name], bound)
    assert len(errs) > 20
    return errs


def _ragged(masked):
    x = _inputs()
    if not masked:
        return x, None
    keep = torch.arange(x.shape[1])[None, :] < LENGTHS[:, None]
    return x * keep, keep.long()


def _graph_nodes(t):
    seen, todo = set(), [t.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        todo += [f for f, _ in fn.next_functions]
    return {type(fn).__name__ for fn in seen}


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_f32_training_forward_and_every_gradient_match_transformers_autograd(family, masked):
    """last_hidden_state (atol 5e-4, rtol 1e-4) and the gradient of EVERY trainable parameter (relative L2 3e-3) of a scalar loss, with and without an
    attention mask (ragged clips: data2vec's stack then carries non-zero padded rows from layer 2 on, as transformers does)."""
    ref, adapt = _pair(family)
    adapt.mask_input = masked
    x, att = _ragged(masked)
    out_ref = ref(x, attention_mask=att).last_hidden_state
    probe = torch.randn(out_ref.shape, generator=torch.Generator().manual_seed(5))
    (out_ref * probe).sum().backward()
    feats, _ = adapt(x.cuda(), LENGTHS.cuda())
    assert feats.shape == (3, out_ref.shape[2], out_ref.shape[1])
    got = feats.transpose(-1, -2)
    np.testing.assert_allclose(got.detach().cpu().numpy(), out_ref.detach().numpy(), atol=5e-4, rtol=1e-4)
    if family.startswith("data2vec"):
        assert "PosConvStackLayerBackward" in _graph_nodes(got)
    (got * probe.cuda()).sum().backward()
    errs = _compare_grads(ref, adapt)
    print(family, masked, "worst gradient error", max(errs.values()))


# ---- what bf16 conv operands do to the gradients of the stack's own parameters: an emulation on the CPU ------------------------------------------
class _Bf16Conv(torch.autograd.Function):
    """Grouped conv1d whose three products read operands rounded to bf16 and accumulate in float64 (results returned in the input's dtype): what the
    matrix-core conv, its data gradient and ts_w2v_posconv_wgrad do, without their f32 accumulation order."""

    @staticmethod
    def forward(ctx, x, w, pad, groups):
        ctx.save_for_backward(x, w)
        ctx.geom = (pad, groups)
        r = lambda v: v.to(torch.bfloat16).double()
        return F.conv1d(r(x), r(w), padding=pad, groups=groups).to(x.dtype)

    @staticmethod
    def backward(ctx, dz):
        x, w = ctx.saved_tensors
        pad, groups = ctx.geom
        r = lambda v: v.to(torch.bfloat16).double()
        with torch.enable_grad():
            xr, wr = r(x).requires_grad_(True), r(w).requires_grad_(True)
            dx, dw = torch.autograd.grad(F.conv1d(xr, wr, padding=pad, groups=groups), (xr, wr), r(dz))
        return dx.to(x.dtype), dw.to(w.dtype), None, None


@contextlib.contextmanager
def _bf16_stack_convs(model):
    """Inside: every conv of the model's positional stack multiplies bf16-rounded operands (its bias is added in the conv's dtype, as before)."""
    convs = [layer.conv for layer in model.encoder.pos_conv_embed.layers]
    old = [c.forward for c in convs]
    for c in convs:
        c.forward = (lambda c_: lambda x: _Bf16Conv.apply(x, c_.weight, c_.padding[0], c_.groups) + c_.bias[None, :, None])(c)
    try:
        yield
    finally:
        for c, f in zip(convs, old):
            c.forward = f


def _emulated_stack_errors(family):
    """{parameter of pos_conv_embed.layers: relative L2 error of its gradient} when only the stack's convs read bf16 operands, against f32 autograd, on the
    masked batch of the tests."""
    x, att = _ragged(True)
    grads = []
    for emulate in (False, True):
        m = _model(family)
        m.feature_extractor._freeze_parameters()
        m.train()
        with (_bf16_stack_convs(m) if emulate else contextlib.nullcontext()):
            out = m(x, attention_mask=att).last_hidden_state
            (out * torch.randn(out.shape, generator=torch.Generator().manual_seed(5))).sum().backward()
        grads.append({n: p.grad for n, p in m.named_parameters() if "pos_conv_embed.layers" in n})
    return {n: float((grads[1][n] - g).norm() / g.norm()) for n, g in grads[0].items()}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_mixed_precision_training_matches_transformers_autograd_within_bf16_tolerance(family):
    """train_precision="bf16" on the masked batch against f32 autograd through the real model: last_hidden_state within 3e-2 of max(1, max |ref|) and not
    bit-equal to f32; every parameter gradient OUTSIDE data2vec's positional stack within 4e-2 relative L2, the project's mixed-precision bound.

    The stack's own parameters, where its convs run on the matrix cores (the _hd64 geometries; at 16 channels per group they are f32 products and the 4e-2
    bound holds for them like for every parameter under the bf16 encoder): their gradients pass through up to 2 x 3 bf16 convs.  The bound is twice the
    error of the CPU emulation above (bf16-rounded conv operands, float64 accumulation, the rest of the model f32), per parameter, computed in the test; twice,
    because the emulation has neither the kernel's f32 accumulation order nor the bf16 encoder above the stack.  Emulated (allowed), layers 0 | 1 | 2:
      data2vec_k19_hd64  weight 6.50e-3 (1.30e-2) | 5.19e-3 (1.04e-2) | 5.19e-3 (1.04e-2)    bias 3.18e-3 (6.4e-3) | 4.23e-3 (8.5e-3) | 3.88e-3 (7.8e-3)
      data2vec_k8_hd64   weight 6.32e-3 (1.26e-2) | 6.35e-3 (1.27e-2) | 5.68e-3 (1.14e-2)    bias 5.62e-3 (1.12e-2) | 5.87e-3 (1.17e-2) | 3.76e-3 (7.5e-3)
    Measured on an MI355X, worst stack parameter: 7.8e-3 of 1.31e-2 allowed (k 19, layers.0 weight), 7.7e-3 of 1.26e-2 (k 8); the parameters outside the stack
    reach 9.3e-3 of their 4e-2.  On the _hd64 geometries the autograd graph holds PosConvStackLayerBackward (data2vec) and AttentionFusedBackward.  The forward is bit-reproducible."""
    ref, adapt = _pair(family)
    adapt.train_precision = "bf16"
    adapt.mask_input = True
    x, att = _ragged(True)
    out_ref = ref(x, attention_mask=att).last_hidden_state
    probe = torch.randn(out_ref.shape, generator=torch.Generator().manual_seed(5))
    (out_ref * probe).sum().backward()
    feats, _ = adapt(x.cuda(), LENGTHS.cuda())
    got = feats.transpose(-1, -2)
    err = float((got.detach().cpu() - out_ref.detach()).abs().max())
    assert err <= 3e-2 * max(1.0, float(out_ref.abs().max())), err
    assert err > 1e-6, "the mixed-precision path did not run (bit-level agreement with f32 is not what bf16 operands give)"
    stack_bound = {}
    if family.endswith("hd64"):
        names = _graph_nodes(got)
        assert "AttentionFusedBackward" in names, names
        if family.startswith("data2vec"):
            assert "PosConvStackLayerBackward" in names, names
            emulated = _emulated_stack_errors(family)
            assert len(emulated) == 6
            assert all(1e-3 < e < 2e-2 for e in emulated.values()), emulated          # the emulation ran, and rounded what it should
            stack_bound = {n: 2.0 * e for n, e in emulated.items()}
            print(family, "emulated", emulated, "allowed", stack_bound)
    (got * probe.cuda()).sum().backward()
    errs = _compare_grads(ref, adapt, tol=4e-2, tol_of=stack_bound.get)
    print(family, "stack gradient errors", {n: e for n, e in errs.items() if "pos_conv_embed" in n}, "worst", max(errs.values()))
    assert max(errs.values()) > 1e-5
    with torch.no_grad():
        feats2, _ = adapt(x.cuda(), LENGTHS.cuda())
    assert torch.equal(feats2, feats)


def test_data2vec_time_masking_follows_transformers_under_the_same_numpy_seed():
    """mask_time_prob > 0: the spans are drawn in front of the stack, as for wav2vec2 -- the same seed masks the same frames; outputs and gradients
    (masked_spec_embed's too) match."""
    ref, adapt = _pair("data2vec_k19", mask_time_prob=0.3, mask_time_length=3, mask_time_min_masks=2)
    x = _inputs(b=2, n=6000, seed=2)
    np.random.seed(11)
    out_ref = ref(x).last_hidden_state
    probe = torch.randn(out_ref.shape, generator=torch.Generator().manual_seed(6))
    (out_ref * probe).sum().backward()
    np.random.seed(11)
    feats, _ = adapt(x.cuda(), torch.tensor([6000, 6000]).cuda())
    got = feats.transpose(-1, -2)
    np.testing.assert_allclose(got.detach().cpu().numpy(), out_ref.detach().numpy(), atol=5e-4, rtol=1e-4)
    (got * probe.cuda()).sum().backward()
    _compare_grads(ref, adapt)
    assert float(adapt.original_encoder.masked_spec_embed.grad.abs().max()) > 0


def test_data2vec_layerdrop_skips_the_same_layers_as_transformers_under_the_same_torch_seed():
    ref, adapt = _pair("data2vec_k19", layerdrop=0.5, num_hidden_layers=4)
    x = _inputs(b=2, n=3000, seed=3)
    torch.manual_seed(21)
    out_ref = ref(x).last_hidden_state
    torch.manual_seed(21)
    feats, _ = adapt(x.cuda(), torch.tensor([3000, 3000]).cuda())
    np.testing.assert_allclose(feats.transpose(-1, -2).detach().cpu().numpy(), out_ref.detach().numpy(), atol=5e-4, rtol=1e-4)


@pytest.mark.parametrize("family", ["data2vec_k19_hd64", "hubert_hd64"])
def test_five_training_steps_through_the_module_lower_the_loss_and_predict_runs_afterwards(family, tmp_path):
    """module_from_huggingface(<family>ForCTC) in mixed precision: five training_step + optimizer steps on one fixed batch; the loss is finite and lower at
    step 5 than at step 1; predict() afterwards runs on the updated weights (the inference plan is re-packed after training)."""
    import json
    from thunder_speech_amd.huggingface.compatibility import module_from_huggingface
    tokens = ["<pad>", "<s>", "</s>", "<unk>", "|"] + [chr(97 + i) for i in range(26)] + ["'"]
    vocab = tmp_path / "vocab.json"
    vocab.write_text(json.dumps({tok: i for i, tok in enumerate(tokens)}))
    tokenizer = transformers.Wav2Vec2CTCTokenizer(str(vocab))
    model = _model(family, seed=3, head=True, vocab_size=len(tokens), pad_token_id=0)
    module = module_from_huggingface(model, transformers.Wav2Vec2FeatureExtractor(return_attention_mask=True), tokenizer)
    module.encoder.train_precision = "bf16"
    module.optimizer_kwargs = {"lr": 1e-3}
    module = module.cuda().train()
    opt = module.configure_optimizers()
    opt = opt["optimizer"] if isinstance(opt, dict) else opt
    batch = (_inputs(b=2, n=8000, seed=7).cuda(), torch.tensor([8000.0, 6000.0]).cuda(), ["hello world", "abc"])
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = module.training_step(batch, 0)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print(family, losses)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    module.eval()
    text = module.predict(batch[0][:1])
    assert isinstance(text, list) and len(text) == 1 and isinstance(text[0], str)
