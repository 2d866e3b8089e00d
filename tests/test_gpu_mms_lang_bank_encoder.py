"""The MMS language bank end to end on the GPU (BaseCTCModule.language_bank, huggingface/language_bank.py, csrc/mms_lang_bank.hip): three languages
on one shared base in one batch against one single-language module per language and against transformers' own logits, eager and from a captured
graph whose selection, and whose bank, change between replays."""
import json
import math
import os

import pytest
import torch

transformers = pytest.importorskip("transformers")

pytestmark = pytest.mark.gpu

# the small MMS config of tests/test_gpu_mms.py (copied: that file is not imported), with a third language
BASE = ["<pad>", "<s>", "</s>", "<unk>", "|"]
VOCABS = {"aaa": BASE + list("abcdefghijklmnopqrstuvwxyz'"), "bbb": BASE + list("zyxwvutsrqpo"), "ccc": BASE + list("0123456789abcdefghi")}
CFG = dict(hidden_size=160, num_hidden_layers=2, num_attention_heads=2, intermediate_size=320, feat_extract_norm="layer", conv_bias=True,
           do_stable_layer_norm=True, vocab_size=len(VOCABS["aaa"]), conv_dim=(32,) * 7, conv_kernel=(10, 3, 3, 3, 3, 2, 2),
           conv_stride=(5, 2, 2, 2, 2, 2, 2), num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, pad_token_id=0, adapter_attn_dim=16,
           layer_norm_eps=1e-3)
SELECTION = ["bbb", None, "ccc", "bbb"]                    # one entry per clip; None: the resident language "aaa"
SERVED = ["bbb", "aaa", "ccc", "bbb"]


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


def _fit_margin_head(model, xn, n_tokens, margin=8.0):
    """lm_head fitted (ridge least squares on transformers' own hidden states) so that every frame's top-1 leads its top-2 by ~`margin`
    (tests/test_gpu_mms.py's, for a vocabulary of n_tokens)."""
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
    w = torch.linalg.solve(hf.T @ hf + 1e-3 * torch.eye(c + 1, dtype=torch.float64), hf.T @ target.double())
    with torch.no_grad():
        model.lm_head.weight.copy_(w[:c].T.float())
        model.lm_head.bias.copy_(w[c].float())


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """A three-language checkpoint directory on one shared base, transformers' logits per language, one single-language module per language,
    and one module with all three in a bank: built once, and only read by the tests (each test leaves the bank and the selection as it found
    them)."""
    from safetensors.torch import save_file
    from thunder_speech_amd.huggingface.compatibility import load_huggingface_checkpoint
    g = torch.Generator().manual_seed(42)
    x = 0.1 * torch.randn(4, 30 * 320 + 80, generator=g)
    n = x.shape[1]
    xn = (x - x.mean(dim=1, keepdim=True)) / torch.sqrt(x.var(dim=1, keepdim=True, unbiased=False) + 1e-7)
    am = torch.ones(4, n, dtype=torch.long)
    models = {lang: _random_mms_ctc(seed, vocab_size=len(VOCABS[lang])) for lang, seed in (("aaa", 43), ("bbb", 41), ("ccc", 45))}
    shared = {k: v for k, v in models["aaa"].state_dict().items() if "adapter_layer" not in k and not k.startswith("lm_head")}
    for lang in ("bbb", "ccc"):
        models[lang].load_state_dict(shared, strict=False)             # one base; the adapters (different seeds) and the heads differ
    ref = {}
    for lang, model in models.items():
        _fit_margin_head(model, xn, len(VOCABS[lang]))
        with torch.no_grad():
            ref[lang] = model(xn, attention_mask=am).logits.transpose(1, 2)
        top2 = ref[lang].topk(2, dim=1).values                          # the margin condition of the two-language test, per language
        assert float((top2[:, 0] - top2[:, 1]).min()) > 0.5 * max(1.0, float(ref[lang].abs().max())), lang
    a0 = models["aaa"].state_dict()["wav2vec2.encoder.layers.0.adapter_layer.linear_2.weight"]
    assert not torch.equal(a0, models["bbb"].state_dict()["wav2vec2.encoder.layers.0.adapter_layer.linear_2.weight"])
    d = str(tmp_path_factory.mktemp("mms_bank"))
    models["aaa"].save_pretrained(d)
    packs = {}
    for lang, model in models.items():
        packs[lang] = {k: v.detach().clone().contiguous() for k, v in model._get_adapters().items()}
        save_file(packs[lang], os.path.join(d, f"adapter.{lang}.safetensors"))
    with open(os.path.join(d, "vocab.json"), "w") as f:
        json.dump({lang: {tok: i for i, tok in enumerate(toks)} for lang, toks in VOCABS.items()}, f)
    transformers.Wav2Vec2CTCTokenizer(os.path.join(d, "vocab.json"), target_lang="aaa").save_pretrained(d)
    transformers.Wav2Vec2FeatureExtractor(return_attention_mask=True).save_pretrained(d)

    single = {lang: load_huggingface_checkpoint(d, target_lang=lang).cuda() for lang in VOCABS}
    m = load_huggingface_checkpoint(d, target_lang="aaa")
    m.language_bank("aaa", capacity=4)                                   # created on the host ...
    assert m.language_bank_load(d, ["bbb", "ccc"]) == [1, 2]
    m = m.cuda()                                                         # ... and moved with the module
    bank = m.__dict__["_language_bank"]
    assert bank.device.type == "cuda" and bank.head_w.is_cuda and m.encoder.__dict__["_language_bank"] is bank
    xc = x.cuda()                                                        # one address: predict()'s zero-copy graph is keyed by it
    lengths = torch.tensor([n] * 4).cuda()
    with torch.no_grad():
        texts = {lang: single[lang].predict(xc) for lang in VOCABS}
    assert all(len(s) > 0 for lang in VOCABS for s in texts[lang])
    return dict(d=d, x=xc, lengths=lengths, ref=ref, single=single, m=m, bank=bank, packs=packs, texts=texts)


def _encode(module, w):
    with torch.no_grad():
        features, feature_lengths = module.audio_transform(w["x"], w["lengths"])
        return module.encoder(features, feature_lengths)[0]


def test_mixed_batch_equals_the_single_language_modules(world):
    w, m = world, world["m"]
    m.select_languages(SELECTION)
    try:
        got = _encode(m, w)
        with torch.no_grad():
            logits, _ = m(w["x"], w["lengths"])
            texts = m.predict(w["x"])
    finally:
        m.select_languages([])
    assert logits.shape == (4, 32, 30)
    outs = {lang: _encode(w["single"][lang], w) for lang in VOCABS}
    assert not torch.equal(outs["aaa"][0], outs["bbb"][0])              # the languages' encoders do differ on the same clip
    for i, lang in enumerate(SERVED):
        assert torch.equal(got[i], outs[lang][i]), f"encoder output of clip {i} ({lang})"
        n = len(VOCABS[lang])
        want = w["ref"][lang][i].argmax(0)
        assert torch.equal(logits[i].argmax(0).cpu(), want) and torch.equal(logits[i, :n].argmax(0).cpu(), want), f"argmax of clip {i} ({lang})"
        assert bool((logits[i, n:].cpu() == torch.tensor(-1e30, dtype=torch.float32)).all())
        assert texts[i] == w["texts"][lang][i]
    with torch.no_grad():
        assert m.predict_languages(w["x"], SELECTION) == texts
    assert m.selected_languages() == []                                  # predict_languages restored the selection


def test_all_resident_equals_the_module_without_a_bank(world):
    w, m = world, world["m"]
    bare = w["single"]["aaa"]
    for selection in ([], ["aaa", None, "aaa"]):
        m.select_languages(selection)
        try:
            with torch.no_grad():
                assert m.predict(w["x"]) == w["texts"]["aaa"]
            assert torch.equal(_encode(m, w), _encode(bare, w))
        finally:
            m.select_languages([])


def test_one_graph_serves_every_selection_and_sees_the_bank_change(world):
    w, m = world, world["m"]
    other = ["ccc", "bbb", None, None]
    want = {tuple(SELECTION): [w["texts"][lang][i] for i, lang in enumerate(SERVED)],
            tuple(other): [w["texts"][lang][i] for i, lang in enumerate(["ccc", "bbb", "aaa", "aaa"])]}
    m.graph_inference = True
    try:
        with torch.no_grad():
            first = [m.predict_languages(w["x"], SELECTION) for _ in range(3)]      # eager, then captured, then replayed
            graphs = m.__dict__.get("_infer_graphs")
            count = graphs[1].count() + graphs[2].count()
            assert count >= 1
            assert first == [want[tuple(SELECTION)]] * 3
            assert m.predict_languages(w["x"], other) == want[tuple(other)]
            assert m.predict_languages(w["x"], SELECTION) == want[tuple(SELECTION)]
            # the bank changes between replays: "ccc" leaves (its clip goes back to the resident language), "bbb"'s pack arrives under a new name
            m.select_languages(other)
            m.language_bank_remove("ccc")
            assert m.selected_languages() == [None, "bbb", None, None]
            assert m.predict(w["x"]) == [w["texts"][lang][i] for i, lang in enumerate(["aaa", "bbb", "aaa", "aaa"])]
            assert m.language_bank_add("bbb2", w["packs"]["bbb"], VOCABS["bbb"]) == 2
            assert m.predict_languages(w["x"], ["bbb2", None, "bbb2", "bbb"]) == [w["texts"][lang][i] for i, lang in enumerate(["bbb", "aaa", "bbb", "bbb"])]
            now = m.__dict__.get("_infer_graphs")
            assert now is graphs and now[1].count() + now[2].count() == count     # nothing was re-captured
    finally:
        m.graph_inference = None
        m.select_languages([])
        if "bbb2" in m.language_bank_names():
            m.language_bank_remove("bbb2")
        if "ccc" not in m.language_bank_names():
            m.language_bank_add("ccc", w["packs"]["ccc"], VOCABS["ccc"])
    assert m.language_bank_names() == ["aaa", "bbb", "ccc"]


def test_align_refuses_a_mixed_selection_and_serves_the_resident_one(world):
    w, m = world, world["m"]
    bare = w["single"]["aaa"]
    texts = w["texts"]["aaa"]
    m.select_languages(SELECTION)
    try:
        with pytest.raises(NotImplementedError, match="align.*language bank"):
            m.align(w["x"], texts)
    finally:
        m.select_languages([])
    got, want = m.align(w["x"], texts), bare.align(w["x"], texts)
    # The two heads multiply the same bf16 operands and differ in the order of an f32 sum of c exact products: a logit moves by at most
    # c 2^-24 S, S = max_v sum_k |W[v][k]| max|h|, and a log-probability by at most twice that; a clip's score sums its frames'.
    head = bare.decoder[2]
    s = float(head.weight.detach().abs().sum(1).max()) * float(_encode(bare, w).abs().max())
    eps = 2 * 160 * 2.0 ** -24 * s
    for a, b in zip(got, want):
        assert [(t.token, t.start_frame, t.end_frame, t.start, t.end) for t in a.tokens] == [(t.token, t.start_frame, t.end_frame, t.start, t.end) for t in b.tokens]
        assert len(a.tokens) > 0 and abs(a.score - b.score) <= 30 * eps
        assert all(abs(ta.logp - tb.logp) <= (tb.end_frame - tb.start_frame) * eps for ta, tb in zip(a.tokens, b.tokens))
