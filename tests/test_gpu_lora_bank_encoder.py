"""GPU checks of the LoRA bank through HuggingFaceEncoderAdapt (lora_bank / lora_bank_add / select_adapters, Wav2Vec2Plan._bank_term on
csrc/lora_bank.hip): every clip of a mixed selection against `transformers`' model on the CPU in f32 whose target nn.Linears are wrapped by a plain
torch module that adds s (x A^T) B^T for that clip's adaptation; the bit-exact properties of the selection; and a captured graph that keeps serving
while the selection and the bank change.  The tiny geometry of tests/test_gpu_lora_finetune.py (hidden 128, 2 layers, 2 heads, short conv stack).
Bounds: precision="fp32" atol 5e-4, rtol 1e-4 and precision="bf16" max <= 0.03 max(1, max|ref|), rms <= 0.006 max(1, max|ref|) -- the project's
encoder bounds (tests/test_gpu_w2v_encoder.py)."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
transformers = pytest.importorskip("transformers")

BASE = dict(vocab_size=32, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, conv_dim=(32, 32, 32),
            conv_stride=(5, 2, 2), conv_kernel=(10, 3, 2), num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=2, hidden_dropout=0.0,
            activation_dropout=0.0, attention_dropout=0.0, feat_proj_dropout=0.0, final_dropout=0.0, layerdrop=0.0, mask_time_prob=0.0,
            mask_feature_prob=0.0)
FAMILIES = {"postln": dict(feat_extract_norm="group", do_stable_layer_norm=False, conv_bias=False),
            "preln": dict(feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True),
            "preln_hd80": dict(feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True, hidden_size=160, intermediate_size=320,
                               num_conv_pos_embedding_groups=4)}
QV, ALL = ("q_proj", "v_proj"), ("q_proj", "k_proj", "v_proj", "out_proj")
RANK = 8
ALPHAS = {"a": 16.0, "b": 8.0, "c": 24.0}              # "a" is added without an alpha: the bank's alpha_default
LENGTHS = [4000, 3000, 2111]
MIXED = ["a", None, "c"]


def _model(family, seed=0):
    torch.manual_seed(seed)
    m = transformers.Wav2Vec2Model(transformers.Wav2Vec2Config(**{**BASE, **FAMILIES[family]}))
    with torch.no_grad():                       # tests/test_gpu_lora_finetune.py::_model: make every parameter matter
        for n, p in m.named_parameters():
            if p.dim() == 1 and "bias" in n:
                p.add_(0.05 * torch.randn_like(p))
            elif "layer_norm.weight" in n:
                p.mul_(1.0 + 0.1 * torch.randn_like(p))
    return m.eval()


def _clips():
    x = torch.randn(3, 4000, generator=torch.Generator().manual_seed(1))
    lengths = torch.tensor(LENGTHS)
    valid = torch.arange(x.shape[1])[None, :] < lengths[:, None]
    return x * valid, lengths, valid.long()


class _LoRAWrapped(torch.nn.Module):
    """The reference: nn.Linear plus s (x A^T) B^T in plain torch (tests/test_gpu_lora_finetune.py)."""

    def __init__(self, lin, a, b, s):
        super().__init__()
        self.lin, self.s = lin, s
        self.lora_A, self.lora_B = torch.nn.Parameter(a.detach().cpu().clone()), torch.nn.Parameter(b.detach().cpu().clone())

    def forward(self, x):
        return self.lin(x) + self.s * ((x @ self.lora_A.T) @ self.lora_B.T)


_ADAPTATIONS, _REFERENCES = {}, {}


def _adaptations(family, targets):
    """{name: what lora_state_dict() exports}: three random adaptations with non-zero B, each made by lora_finetuning() on a throw-away copy."""
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    key = (family, targets)
    if key not in _ADAPTATIONS:
        out = {}
        for seed, name in enumerate(ALPHAS):
            throw = HuggingFaceEncoderAdapt(_model(family), train_precision="bf16")
            torch.manual_seed(100 + seed)
            named = throw.lora_finetuning(rank=RANK, alpha=ALPHAS[name], targets=targets)
            g = torch.Generator().manual_seed(3 + seed)
            with torch.no_grad():
                for n, p in named.items():
                    if n.endswith("lora_B"):
                        p.copy_(0.1 * torch.randn(p.shape, generator=g))
            out[name] = throw.lora_state_dict()
        _ADAPTATIONS[key] = out
    return _ADAPTATIONS[key]


def _reference(family, targets):
    """{name or None: last_hidden_state [3][T][C] of transformers on the CPU with every clip under that adaptation}, computed once."""
    key = (family, targets)
    if key not in _REFERENCES:
        x, _, att = _clips()
        base = _model(family)
        with torch.no_grad():
            outs = {None: base(x, attention_mask=att).last_hidden_state}
            for name, sd in _adaptations(family, targets).items():
                m = copy.deepcopy(base)
                for i, layer in enumerate(m.encoder.layers):
                    for t in targets:
                        q = f"lora.layers.{i}.{t}."
                        setattr(layer.attention, t, _LoRAWrapped(getattr(layer.attention, t), sd[q + "lora_A"], sd[q + "lora_B"], ALPHAS[name] / RANK))
                outs[name] = m(x, attention_mask=att).last_hidden_state
        _REFERENCES[key] = outs
    return _REFERENCES[key]


def _encoder(family, precision):
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    return HuggingFaceEncoderAdapt(_model(family), mask_input=True, precision=precision).cuda().eval()


def _fill(enc, family, targets, capacity=4):
    enc.lora_bank(rank=RANK, alpha_default=ALPHAS["a"], targets=targets, capacity=capacity)
    for name, sd in _adaptations(family, targets).items():
        enc.lora_bank_add(name, sd, alpha=None if name == "a" else ALPHAS[name])


def _run(enc):
    x, lengths, _ = _clips()
    with torch.no_grad():
        feats, _ = enc(x.cuda(), lengths.cuda())
    return feats.transpose(-1, -2).float().cpu()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("targets", [QV, ALL], ids=["qv", "all"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_each_clip_of_a_mixed_selection_matches_transformers_under_its_adaptation(family, targets, precision):
    refs = _reference(family, targets)
    enc = _encoder(family, precision)
    _fill(enc, family, targets)
    enc.select_adapters(MIXED)
    got = _run(enc)
    for i, name in enumerate(MIXED):
        ref, base = refs[name][i], refs[None][i]
        err = (got[i] - ref).abs()
        scale = max(1.0, float(ref.abs().max()))
        rms = float((got[i] - ref).pow(2).mean().sqrt())
        err_base = float((got[i] - base).abs().max())
        print(f"{family} {precision} {'+'.join(t[0] for t in targets)} clip {i} ({name}): max err {float(err.max()):.3e} rms {rms:.3e} against scale "
              f"{scale:.3e}; against the base-only reference {err_base:.3e}")
        if precision == "fp32":
            assert bool((err <= 5e-4 + 1e-4 * ref.abs()).all()), float((err - 5e-4 - 1e-4 * ref.abs()).max())
        else:
            assert float(err.max()) <= 0.03 * scale and rms <= 0.006 * scale
        if name is not None:
            assert err_base > float(err.max()), "the bank did not run for this clip"


@pytest.mark.parametrize("family,precision,targets", [("postln", "bf16", ALL), ("preln", "bf16", QV), ("preln_hd80", "bf16", ALL), ("preln", "fp32", ALL)])
def test_selection_is_exact_per_clip(family, precision, targets):
    enc = _encoder(family, precision)
    before = _run(enc)
    _fill(enc, family, targets)
    assert torch.equal(_run(enc), before)                                    # after lora_bank(): every clip runs the base alone, bit for bit
    enc.select_adapters([None, None, None])
    assert torch.equal(_run(enc), before)
    enc.select_adapters(MIXED)
    mixed = _run(enc)
    assert torch.equal(mixed[1], before[1]) and not torch.equal(mixed[0], before[0]) and not torch.equal(mixed[2], before[2])
    for i, name in enumerate(MIXED):
        enc.select_adapters([name] * 3)
        assert torch.equal(_run(enc)[i], mixed[i]), (i, name)                # a clip's result depends on its own selection only
    # remove, then add the same tensors again (into whichever slot is free): equal bits
    enc.select_adapters(MIXED)
    enc.lora_bank_remove("a")
    assert enc.selected_adapters() == [None, None, "c"]
    gone = _run(enc)
    assert torch.equal(gone[0], before[0]) and torch.equal(gone[2], mixed[2])
    enc.lora_bank_add("extra", _adaptations(family, targets)["b"], alpha=3.0)        # takes the freed slot
    enc.lora_bank_add("a", _adaptations(family, targets)["a"])
    enc.select_adapters(MIXED)
    assert torch.equal(_run(enc), mixed)


def _module(family="postln", hidden=128):
    """A CTC module whose encoder got its bank on the host, before .cuda(): the bank follows the module to the device."""
    from thunder_speech_amd.blocks import linear_decoder
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    from thunder_speech_amd.huggingface.transform import Wav2Vec2Preprocess
    from thunder_speech_amd.module import BaseCTCModule
    from thunder_speech_amd.text_processing.transform import BatchTextTransformer
    enc = HuggingFaceEncoderAdapt(_model(family, seed=3), precision="bf16")
    enc.lora_bank(rank=RANK, alpha_default=ALPHAS["a"], targets=QV, capacity=4)
    sds = _adaptations(family, QV)
    enc.lora_bank_add("a", sds["a"])
    enc.lora_bank_add("b", sds["b"], alpha=ALPHAS["b"])
    tokens = [chr(97 + i) for i in range(26)] + [" "]
    torch.manual_seed(4)
    module = BaseCTCModule(enc, linear_decoder(hidden, len(tokens) + 1, 0.0), Wav2Vec2Preprocess(), BatchTextTransformer(tokens=tokens)).cuda().eval()
    assert enc._lora_bank.ids.is_cuda and enc._lora_bank.a_qkv.is_cuda and enc.lora_bank_names() == ["a", "b"]
    return module, sds


def test_a_captured_graph_serves_a_new_selection_and_a_new_adaptation():
    module, sds = _module()
    enc = module.encoder
    module.graph_inference = True
    x = torch.randn(2, 8000, generator=torch.Generator().manual_seed(7)).cuda()
    lengths = torch.tensor([8000, 8000]).cuda()

    def eager():
        module.graph_inference = False
        try:
            return module(x, lengths)[0]
        finally:
            module.graph_inference = True

    with torch.no_grad():
        enc.select_adapters(["a", None])
        first = [module(x, lengths)[0] for _ in range(3)]                    # eager, then captured, then replayed
        graphs = module.__dict__.get("_infer_graphs")
        assert graphs is not None and graphs[1].count() + graphs[2].count() >= 1
        count = graphs[1].count() + graphs[2].count()
        assert torch.equal(first[0], first[1]) and torch.equal(first[1], first[2])
        enc.select_adapters(["b", "a"])
        assert enc.lora_bank_add("c", sds["c"], alpha=ALPHAS["c"]) == 2
        second = module(x, lengths)[0]
        assert module.__dict__.get("_infer_graphs") is graphs and graphs[1].count() + graphs[2].count() == count       # replayed, not rebuilt
        assert not torch.equal(second, first[0]) and torch.equal(second, eager())
        enc.select_adapters(["c", "b"])                                      # the adaptation that arrived after the capture
        third = module(x, lengths)[0]
        assert not torch.equal(third[0], second[0]) and torch.equal(third, eager())
        # predict_adapted: selects, predicts, and puts the previous selection back
        texts = module.predict_adapted(x, ["a", "c"])
        assert enc.selected_adapters() == ["c", "b"] and enc._lora_bank.ids[:3].tolist() == [2, 1, -1]
        assert torch.equal(module(x, lengths)[0], third)
        enc.select_adapters(["a", "c"])
        assert module.predict(x) == texts and len(texts) == 2 and all(isinstance(t, str) for t in texts)
        # predict() makes int32 lengths of its own: another input signature, so it may capture a graph of its own next to the first -- in the
        # same table, which none of the above rebuilt
        assert module.__dict__.get("_infer_graphs") is graphs and graphs[1].count() + graphs[2].count() >= count
