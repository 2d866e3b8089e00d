"""GPU parity of LoRA fine-tuning (huggingface/train.py's LoRALinear on csrc/lora_train.hip, through HuggingFaceEncoderAdapt.lora_finetuning()) against
`transformers`' model on the CPU in f32 whose target nn.Linears are wrapped by a plain torch module that adds s (x A^T) B^T, under torch autograd.
The tiny geometry of tests/test_gpu_w2v_train.py (hidden 128, 2 layers, 2 heads, short conv stack), every dropout, LayerDrop and mask_time_prob at 0.
Bounds: outputs within 3e-2 of the reference's scale, every A / B gradient within 4e-2 -- the OUT_TOL / GRAD_TOL pair of
tests/test_gpu_conformer_train.py, with the gradient floor of tests/test_gpu_mms_adapter_train.py (1e-4 of the model's largest gradient)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
transformers = pytest.importorskip("transformers")

OUT_TOL, GRAD_TOL = 3e-2, 4e-2
BASE = dict(vocab_size=32, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, conv_dim=(32, 32, 32),
            conv_stride=(5, 2, 2), conv_kernel=(10, 3, 2), num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=2, hidden_dropout=0.0,
            activation_dropout=0.0, attention_dropout=0.0, feat_proj_dropout=0.0, final_dropout=0.0, layerdrop=0.0, mask_time_prob=0.0,
            mask_feature_prob=0.0)
FAMILIES = {"postln": dict(feat_extract_norm="group", do_stable_layer_norm=False, conv_bias=False),
            "preln": dict(feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True),
            # head_dim 80: the AttentionFused80 neighbour
            "preln_hd80": dict(feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True, hidden_size=160, intermediate_size=320,
                               num_conv_pos_embedding_groups=4)}
QV, ALL = ("q_proj", "v_proj"), ("q_proj", "k_proj", "v_proj", "out_proj")
RANK, ALPHA = 8, 16.0
LENGTHS = [4000, 3000, 2111]


def _model(family, seed=0, cls="Wav2Vec2", **over):
    torch.manual_seed(seed)
    m = getattr(transformers, cls + "Model")(getattr(transformers, cls + "Config")(**{**BASE, **FAMILIES[family], **over}))
    with torch.no_grad():                       # tests/test_gpu_w2v_train.py::_model: make every parameter matter
        for n, p in m.named_parameters():
            if p.dim() == 1 and "bias" in n:
                p.add_(0.05 * torch.randn_like(p))
            elif "layer_norm.weight" in n:
                p.mul_(1.0 + 0.1 * torch.randn_like(p))
    return m


def _clips():
    x = torch.randn(3, 4000, generator=torch.Generator().manual_seed(1))
    lengths = torch.tensor(LENGTHS)
    valid = torch.arange(x.shape[1])[None, :] < lengths[:, None]
    return x * valid, lengths, valid.long()


class _LoRAWrapped(torch.nn.Module):
    """The reference: nn.Linear plus s (x A^T) B^T in plain torch."""

    def __init__(self, lin, a, b, s):
        super().__init__()
        self.lin, self.s = lin, s
        self.lora_A, self.lora_B = torch.nn.Parameter(a.detach().cpu().clone()), torch.nn.Parameter(b.detach().cpu().clone())

    def forward(self, x):
        return self.lin(x) + self.s * ((x @ self.lora_A.T) @ self.lora_B.T)


def _random_b(named, seed=3):
    """B random and non-zero, so that A has a gradient."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in named.items():
            if n.endswith("lora_B"):
                p.copy_((0.1 * torch.randn(p.shape, generator=g)).to(p.device))


def _pair(family, targets, cls="Wav2Vec2", **over):
    """(the wrapped reference on the CPU as a call (x, attention_mask) -> last_hidden_state, its LoRA parameters by our names, the adapter on the
    GPU, its LoRA parameters): the same weights."""
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    ref = _model(family, cls=cls, **over)
    mine = _model(family, cls=cls, **over)
    mine.load_state_dict(ref.state_dict())
    adapt = HuggingFaceEncoderAdapt(mine, mask_input=True, precision="fp32", train_precision="bf16").cuda()
    named = adapt.lora_finetuning(rank=RANK, alpha=ALPHA, targets=targets)
    _random_b(named)
    for p in ref.parameters():
        p.requires_grad_(False)
    theirs = {}
    ref.train()
    if cls == "WavLM":
        # WavLMAttention hands q_proj.weight & co. to F.multi_head_attention_forward instead of calling the Linear, so a wrapper is never run:
        # the same f32 function with the effective weights W + s B A formed under autograd and substituted into the call
        theirs = {n: torch.nn.Parameter(p.detach().cpu().clone()) for n, p in named.items()}

        def run(x, att):
            sub = {}
            for i in range(len(ref.encoder.layers)):
                for t in targets:
                    q, key = f"lora.layers.{i}.{t}.", f"encoder.layers.{i}.attention.{t}.weight"
                    sub[key] = ref.get_parameter(key).detach() + (ALPHA / RANK) * (theirs[q + "lora_B"] @ theirs[q + "lora_A"])
            return torch.func.functional_call(ref, sub, (x,), dict(attention_mask=att)).last_hidden_state
        return run, theirs, adapt.train(), named
    for i, layer in enumerate(ref.encoder.layers):
        for t in targets:
            q = f"lora.layers.{i}.{t}."
            wrapped = _LoRAWrapped(getattr(layer.attention, t), named[q + "lora_A"], named[q + "lora_B"], ALPHA / RANK)
            setattr(layer.attention, t, wrapped)
            theirs[q + "lora_A"], theirs[q + "lora_B"] = wrapped.lora_A, wrapped.lora_B
    return (lambda x, att: ref(x, attention_mask=att).last_hidden_state), theirs, adapt.train(), named


def _graph(fn):
    seen, todo = set(), [fn]
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        todo += [g for g, _ in f.next_functions]
    return seen


def _check_parity(family, targets, cls="Wav2Vec2", attention_node=None, **over):
    x, lengths, att = _clips()
    ref, theirs, adapt, named = _pair(family, targets, cls=cls, **over)
    assert len(named) == 2 * 2 * len(targets)
    out_ref = ref(x, att)
    probe = torch.randn(out_ref.shape, generator=torch.Generator().manual_seed(5))
    (out_ref * probe).sum().backward()
    feats, _ = adapt(x.cuda(), lengths.cuda())
    got = feats.transpose(-1, -2)
    err, scale = float((got.detach().cpu() - out_ref.detach()).abs().max()), float(out_ref.detach().abs().max())
    print(f"{cls} {family} {targets}: output max abs error {err:.3e} against scale {scale:.3e}")
    assert err <= OUT_TOL * max(1.0, scale), err
    assert err > 1e-6, "the mixed-precision path did not run"
    nodes = _graph(got.grad_fn)
    names = {type(f).__name__ for f in nodes}
    assert "LoRALinearBackward" in names, names
    if attention_node is not None:
        assert attention_node in names, names
    (got * probe.cuda()).sum().backward()
    # every base parameter: no gradient at all
    for n, p in adapt.original_encoder.named_parameters():
        assert p.grad is None and not p.requires_grad, n
    floor2 = 1e-4 * max(float(p.grad.norm()) for p in theirs.values())
    floor_max = 1e-4 * max(float(p.grad.abs().max()) for p in theirs.values())
    for n, p in theirs.items():
        q = named[n]
        assert p.grad is not None and q.grad is not None and q.grad.shape == p.grad.shape, n
        d = q.grad.cpu() - p.grad
        r2 = float(d.norm()) / max(float(p.grad.norm()), floor2)
        rmax = float(d.abs().max()) / max(float(p.grad.abs().max()), floor_max)
        print(f"    {n}: relative gradient error {rmax:.3e} (max-norm) {r2:.3e} (L2)")
        assert float(p.grad.abs().max()) > 0, n
        assert rmax <= GRAD_TOL and r2 <= GRAD_TOL, (n, rmax, r2)


@pytest.mark.parametrize("targets", [QV, ALL], ids=["qv", "qkvo"])
@pytest.mark.parametrize("family", ["postln", "preln"])
def test_outputs_and_lora_gradients_match_the_wrapped_transformers_model(family, targets):
    _check_parity(family, targets, attention_node="AttentionFusedBackward")


def test_head_dim_80_takes_the_fused_attention_neighbour():
    _check_parity("preln_hd80", ALL, attention_node="AttentionFused80Backward")


def test_wavlm_trains_lora_through_the_same_chain():
    _check_parity("preln", QV, cls="WavLM", attention_node="WavLMAttentionFusedBackward", num_buckets=32, max_bucket_distance=40)


def test_with_b_zero_the_train_output_is_the_plain_adapters_bit_for_bit():
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    x, lengths, _ = _clips()
    adapt = HuggingFaceEncoderAdapt(_model("postln"), mask_input=True, precision="fp32", train_precision="bf16").cuda().train()
    before, _ = adapt(x.cuda(), lengths.cuda())
    assert "LoRALinearBackward" not in {type(f).__name__ for f in _graph(before.grad_fn)}
    named = adapt.lora_finetuning(rank=RANK, alpha=ALPHA, targets=ALL)
    after, _ = adapt(x.cuda(), lengths.cuda())
    assert "LoRALinearBackward" in {type(f).__name__ for f in _graph(after.grad_fn)}
    assert torch.equal(after.detach(), before.detach())
    _random_b(named)
    moved, _ = adapt(x.cuda(), lengths.cuda())
    assert not torch.equal(moved.detach(), before.detach())


def _module(family="postln", hidden=128):
    from thunder_speech_amd.blocks import linear_decoder
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    from thunder_speech_amd.huggingface.transform import Wav2Vec2Preprocess
    from thunder_speech_amd.module import BaseCTCModule
    from thunder_speech_amd.text_processing.transform import BatchTextTransformer
    enc = HuggingFaceEncoderAdapt(_model(family, seed=3), precision="fp32", train_precision="bf16")
    tokens = [chr(97 + i) for i in range(26)] + [" "]
    torch.manual_seed(4)
    # SGD's step size: the CTC loss is summed over the batch, so a head weight's gradient is a sum over ~50 frames of (softmax - target) x feature
    # with |feature|^2 ~ 128 x O(1); one step moves a frame's logits by about lr x 128 x (a few correlated frames).  2e-4 keeps that near 0.1, well
    # inside the region where plain gradient descent on a softmax loss descends (0.05 moves logits by tens and diverges)
    return BaseCTCModule(enc, linear_decoder(hidden, len(tokens) + 1, 0.0), Wav2Vec2Preprocess(), BatchTextTransformer(tokens=tokens),
                         optimizer_class=torch.optim.SGD, optimizer_kwargs={"lr": 2e-4}).cuda()


def test_ten_sgd_steps_lower_the_loss_move_predict_and_merge_is_bit_equal():
    module = _module()
    enc = module.encoder
    named = enc.lora_finetuning(rank=RANK, alpha=ALPHA, targets=ALL)
    opt = module.configure_optimizers()
    assert isinstance(opt, torch.optim.SGD)
    x = torch.randn(2, 8000, generator=torch.Generator().manual_seed(7)).cuda()
    lengths = torch.tensor([8000, 8000]).cuda()
    batch = (x, torch.tensor([8000.0, 6000.0]).cuda(), ["hello world", "abc"])
    base = {n: p.detach().clone() for n, p in enc.original_encoder.named_parameters()}
    module.eval()
    with torch.no_grad():
        logits0, _ = module(x, lengths)
    module.train()
    losses = []
    for _ in range(10):
        opt.zero_grad()
        loss = module.training_step(batch, 0)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print("CTC loss over ten SGD steps:", " ".join(f"{v:.4f}" for v in losses))
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0]
    for n, p in enc.original_encoder.named_parameters():
        assert p.grad is None and torch.equal(p.detach(), base[n]), n
    assert all(float(p.detach().abs().max()) > 0 for p in named.values())            # B left zero, A moved with it
    module.eval()
    with torch.no_grad():
        texts = module.predict(x)
        logits1, _ = module(x, lengths)
        f1, _ = enc(x, lengths)
    assert len(texts) == 2 and all(isinstance(t, str) for t in texts)
    assert bool(torch.isfinite(logits1.float()).all()) and not torch.equal(logits1, logits0)      # no stale plan
    # the encoder's share of that: with the LoRA pairs back at zero the features are the untouched base's
    enc.merge_lora()
    assert not hasattr(enc, "lora")
    with torch.no_grad():
        logits2, _ = module(x, lengths)
        f2, _ = enc(x, lengths)
        texts2 = module.predict(x)
    assert torch.equal(f2, f1) and torch.equal(logits2, logits1) and texts2 == texts
    assert any(not torch.equal(p.detach(), base[n]) for n, p in enc.original_encoder.named_parameters())


def test_a_graphed_predict_sees_a_step_on_the_lora_pairs():
    module = _module().eval()
    named = module.encoder.lora_finetuning(rank=RANK, alpha=ALPHA, targets=QV)
    _random_b(named)
    module.graph_inference = True
    x = torch.randn(2, 8000, generator=torch.Generator().manual_seed(7)).cuda()
    lengths = torch.tensor([8000, 8000]).cuda()
    with torch.no_grad():
        first = [module(x, lengths)[0] for _ in range(3)]                  # eager, then captured, then replayed
        graphs = module.__dict__.get("_infer_graphs")
        assert graphs is not None and graphs[1].count() + graphs[2].count() >= 1
        assert torch.equal(first[0], first[1]) and torch.equal(first[1], first[2])
        for n, p in named.items():                                          # what an optimizer step does: in place, no train() / eval() in between
            if n.endswith("lora_B"):
                p.mul_(-1.0)
        second = [module(x, lengths)[0] for _ in range(3)]
    assert not torch.equal(second[0], first[0])
    assert torch.equal(second[0], second[1]) and torch.equal(second[1], second[2])
