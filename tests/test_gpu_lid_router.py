"""The language router end to end on the GPU (BaseCTCModule.language_router / identify_languages / predict_auto, huggingface/language_bank.py):
an audio classifier writes every clip's bank slot on the device and the ASR forward behind it reads them, all from ONE captured graph.

The classifier is built from transformers' own numbers so that every clip has an intended class: with p_b the reference's f32 pooled projected
vector of clip b and d_b = p_b - mean_b p_b, the intended class's row is 0.05 randn + 6 d_b / |d_b|^2 (summed over the clips that intend it) and
the bias is -W mean_b p_b; the clip whose intended class belongs to a language the bank lacks gets a second row at half that height, of a
language the bank holds.  The test asserts its own conditions: the reference's top-1 margin on every clip, global and restricted to the
bank's classes, is at least 10 x the deviation max |HIP - reference| it measures; if that ever fails the inputs are wrong, not the tolerance."""
import copy
import math

import pytest
import torch

transformers = pytest.importorskip("transformers")

pytestmark = pytest.mark.gpu

# the small MMS config of tests/test_gpu_mms_lang_bank_encoder.py (copied: that file is not imported)
BASE = ["<pad>", "<s>", "</s>", "<unk>", "|"]
VOCABS = {"aaa": BASE + list("abcdefghijklmnopqrstuvwxyz'"), "bbb": BASE + list("zyxwvutsrqpo"), "ccc": BASE + list("0123456789abcdefghi"),
          "ddd": BASE + list("mnopqrstuvw")}
CFG = dict(hidden_size=160, num_hidden_layers=2, num_attention_heads=2, intermediate_size=320, feat_extract_norm="layer", conv_bias=True,
           do_stable_layer_norm=True, vocab_size=len(VOCABS["aaa"]), conv_dim=(32,) * 7, conv_kernel=(10, 3, 3, 3, 3, 2, 2),
           conv_stride=(5, 2, 2, 2, 2, 2, 2), num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, pad_token_id=0, adapter_attn_dim=16,
           layer_norm_eps=1e-3)
N = 16000                                                               # four 1 s clips: noise plus a tone each
TONES = (200.0, 900.0, 2500.0, 5000.0)
LABELS = [f"c{i:02d}" for i in range(12)]
INTENDED = [7, 2, 9, 2]
SECOND = (2, 4)                                                         # clip 2's second-best class: c04, the resident language's
# three labels mapped to the bank's languages; the class clip 2 intends belongs to a language the bank does not hold at first
MAPPING = {"c07": "bbb", "c02": "ccc", "c04": "aaa", "c09": "ddd"}
SELECTION = ["ccc", None, None, "bbb"]                                  # what select_languages holds around the routed calls


class _Tok:
    """The two things text_transform_from_tokenizer reads of a tokenizer."""
    pad_token, unk_token, additional_special_tokens = "<pad>", "<unk>", []

    def __init__(self, tokens):
        self.tokens = tokens

    def get_vocab(self):
        return {t: i for i, t in enumerate(self.tokens)}


def _random_mms_ctc(seed, **kw):
    """tests/test_gpu_mms_lang_bank_encoder.py's: biases 0.1 randn, adapters of the order of the residual stream."""
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
        model.lm_head.weight.copy_(4.0 * torch.randn_like(model.lm_head.weight) / math.sqrt(model.lm_head.weight.shape[1]))
    return model


def _classifier_model(xn, am):
    """The same geometry without adapters, classifier_proj_size 64, 12 labels; seed 3.  -> (model, reference f32 logits on the CPU)."""
    torch.manual_seed(3)
    cfg = transformers.Wav2Vec2Config(**{**CFG, "adapter_attn_dim": None}, classifier_proj_size=64, num_labels=len(LABELS),
                                      id2label=dict(enumerate(LABELS)), label2id={s: i for i, s in enumerate(LABELS)})
    model = transformers.Wav2Vec2ForSequenceClassification(cfg).eval()
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if k.endswith(".bias"):
                v.copy_(0.1 * torch.randn(v.shape, generator=g))
        model.projector.weight.copy_(torch.randn(model.projector.weight.shape, generator=g) / math.sqrt(160))
        p = model.projector(model.wav2vec2(xn, attention_mask=am).last_hidden_state).mean(1)          # full-length clips: the plain mean
        mean = p.mean(0)
        d = p - mean
        w = 0.05 * torch.randn(len(LABELS), 64, generator=g)
        for b, k in enumerate(INTENDED):
            w[k] += 6 * d[b] / d[b].pow(2).sum()
        # clip 2's intended class belongs to a language the bank does not hold at first: the same recipe at half the height gives that clip a
        # second-best class of a language it does hold, so the reference's RESTRICTED arg-max has a margin there too
        w[SECOND[1]] += 3 * d[SECOND[0]] / d[SECOND[0]].pow(2).sum()
        model.classifier.weight.copy_(w)
        model.classifier.bias.copy_(-(w @ mean))
        ref = model(xn, attention_mask=am).logits
    return model, ref


@pytest.fixture(scope="module")
def world():
    from thunder_speech_amd.huggingface import classifier_from_huggingface
    from thunder_speech_amd.huggingface.compatibility import module_from_huggingface
    g = torch.Generator().manual_seed(11)
    tt = torch.arange(N) / 16000.0
    x = torch.stack([0.1 * torch.randn(N, generator=g) + 0.5 * torch.sin(2 * math.pi * f * tt) for f in TONES])
    xn = (x - x.mean(dim=1, keepdim=True)) / torch.sqrt(x.var(dim=1, keepdim=True, unbiased=False) + 1e-7)
    am = torch.ones(4, N, dtype=torch.long)
    clf_model, ref = _classifier_model(xn, am)
    assert ref.argmax(1).tolist() == INTENDED
    fe = transformers.Wav2Vec2FeatureExtractor(return_attention_mask=True)
    clf = classifier_from_huggingface(copy.deepcopy(clf_model), fe).cuda()

    models = {lang: _random_mms_ctc(seed, vocab_size=len(VOCABS[lang])) for lang, seed in (("aaa", 43), ("bbb", 41), ("ccc", 45), ("ddd", 47))}
    packs = {lang: {k: v.detach().clone() for k, v in models[lang]._get_adapters().items()} for lang in ("bbb", "ccc", "ddd")}
    m = module_from_huggingface(models["aaa"], fe, _Tok(VOCABS["aaa"]))
    m.language_bank("aaa", capacity=4)
    for lang in ("bbb", "ccc"):                                        # three languages in the bank
        m.language_bank_add(lang, packs[lang], VOCABS[lang])
    m = m.cuda()
    m.language_router(clf, MAPPING)
    xc = x.cuda()
    lengths = torch.full((4,), N, dtype=torch.int32, device="cuda")
    with torch.no_grad():
        got = clf(xc, lengths).double().cpu()
    dev = float((got - ref.double()).abs().max())
    top2 = ref.topk(2, dim=1).values
    margin = float((top2[:, 0] - top2[:, 1]).min())
    print(f"router: reference top-1 margins {[round(float(v), 2) for v in top2[:, 0] - top2[:, 1]]}, logit scale {float(ref.abs().max()):.1f}, "
          f"max |HIP - reference| {dev:.4f}")
    assert margin >= 10 * dev, (margin, dev)                            # the test's own condition: else the inputs are wrong
    for names in (["aaa", "bbb", "ccc"], ["aaa", "bbb", "ccc", "ddd"]):                # and the same for the restricted arg-max, with and without "ddd"
        allowed = [i for i, s in enumerate(LABELS) if MAPPING.get(s) in names]
        r2 = ref[:, allowed].topk(2, dim=1).values
        assert float((r2[:, 0] - r2[:, 1]).min()) >= 10 * dev, (names, r2, dev)
    return dict(m=m, clf=clf, x=xc, lengths=lengths, ref=ref, got=got, packs=packs, bank=m.__dict__["_language_bank"])


def _restricted(logits, bank_names):
    """Per clip the language of the arg-max over the classes mapped to a language in `bank_names`; None when no class is."""
    allowed = [i for i, s in enumerate(LABELS) if MAPPING.get(s) in bank_names]
    if not allowed:
        return [None] * logits.shape[0]
    idx = logits[:, allowed].argmax(1).tolist()
    return [MAPPING[LABELS[allowed[i]]] for i in idx]


def test_identify_languages_is_the_restricted_argmax(world):
    w, m = world, world["m"]
    got = m.identify_languages(w["x"])
    # the reference's restricted arg-max on all four clips, with the margins asserted in the fixture.  Clip 2's intended class belongs to "ddd",
    # which the bank does not hold: the restricted arg-max is -1 only when NO class is allowed, so the clip goes to its best allowed class,
    # the resident language's c04
    assert got == _restricted(w["ref"], m.language_bank_names()) == ["bbb", "ccc", "aaa", "ccc"]
    assert got == _restricted(w["got"], m.language_bank_names())
    assert m.selected_languages() == [] and bool((w["bank"].ids == -1).all())          # identify_languages leaves the id buffer alone
    # no class of the bank's languages: None for every clip (the resident language would serve them)
    m.language_router(w["clf"], {"c09": "ddd", "c11": "eee"})
    try:
        assert m.identify_languages(w["x"]) == [None] * 4
        with torch.no_grad():
            texts, langs = m.predict_auto(w["x"])
            assert langs == ["aaa"] * 4 and texts == m.predict(w["x"])
    finally:
        m.language_router(w["clf"], MAPPING)


def test_predict_auto_serves_the_routed_languages_from_one_graph_and_restores_the_selection(world):
    from thunder_speech_amd.huggingface import language_bank as LB
    w, m, bank = world, world["m"], world["bank"]
    x = w["x"]
    m.select_languages(SELECTION)
    try:
        with torch.no_grad():
            before = m.predict(x)
            routed = m.identify_languages(x)
            texts, langs = m.predict_auto(x)
            graphs = m.__dict__["_auto_graphs"]
            assert graphs[1].count() == 1
            assert langs == routed == _restricted(w["ref"], m.language_bank_names()) == ["bbb", "ccc", "aaa", "ccc"]
            assert m.selected_languages() == SELECTION and bank.ids[:5].tolist() == [2, -1, -1, 1, -1]
            assert m.predict(x) == before
            assert texts == m.predict_languages(x, langs) and all(len(s) > 0 for s in texts)
            assert len(set(m.predict_languages(x, [lang] * 4)[0] for lang in ("aaa", "bbb", "ccc"))) == 3      # the languages do differ

            # the ASR logits of the routed replay against the explicit selection, bit for bit
            logits = LB.auto_forward(m, x)[0].clone()
            assert bank.ids[:4].tolist() == [bank.names.index(s) for s in langs]                                   # written on the device
            bank.write_ids()
            m.select_languages(langs)
            explicit, _ = m(x, w["lengths"])
            m.select_languages(SELECTION)
            assert torch.equal(logits, explicit)
            assert m.__dict__["_auto_graphs"] is graphs and graphs[1].count() == 1

            # the language that was missing arrives: the SAME replay routes clip 2 to it (its class is the clip's global winner) ...
            assert m.language_bank_add("ddd", w["packs"]["ddd"], VOCABS["ddd"]) == 3
            texts2, langs2 = m.predict_auto(x)
            assert langs2 == ["bbb", "ccc", "ddd", "ccc"] == m.identify_languages(x) == _restricted(w["ref"], m.language_bank_names())
            assert texts2 == m.predict_languages(x, langs2) and texts2[2] != texts[2]
            assert [texts2[i] for i in (0, 1, 3)] == [texts[i] for i in (0, 1, 3)]
            # ... and leaves again: back to where the clip was routed before
            m.language_bank_remove("ddd")
            texts3, langs3 = m.predict_auto(x)
            assert (texts3, langs3) == (texts, langs)
            assert m.__dict__["_auto_graphs"] is graphs and graphs[1].count() == 1                             # captured once, replayed throughout
            assert m.selected_languages() == SELECTION and m.predict(x) == before
    finally:
        if "ddd" in m.language_bank_names():
            m.language_bank_remove("ddd")
        m.select_languages([])


def test_predict_auto_follows_the_classifier_when_it_drops_its_device_operands(world):
    """clf.eval() and a redundant clf.cuda() change no parameter but drop the classifier's packed head operands; the next call allocates new ones.
    The routed graph holds the old addresses: it must be captured anew, not replayed on freed memory."""
    w, m, clf = world, world["m"], world["clf"]
    x = w["x"]
    with torch.no_grad():
        first = m.predict_auto(x)
        assert first[1] == ["bbb", "ccc", "aaa", "ccc"]
        for drop in (clf.eval, clf.cuda):
            graphs = m.__dict__["_auto_graphs"]
            epoch = clf.operand_epoch
            shapes = [(t.shape, t.dtype) for k, t in clf.__dict__["_packed"][1].items() if k != "prec"]
            drop()
            assert "_packed" not in clf.__dict__
            # whatever lands in the freed blocks next: values that would turn every logit over
            junk = [torch.full(shape, 1.0e4, dtype=dtype, device="cuda") for shape, dtype in shapes for _ in range(4)]
            torch.cuda.synchronize()
            assert m.predict_auto(x) == first
            assert clf.operand_epoch == epoch + 1 and m.__dict__["_auto_graphs"] is not graphs      # new operands, a new capture
            again = m.__dict__["_auto_graphs"]
            assert m.predict_auto(x) == first and m.__dict__["_auto_graphs"] is again and again[1].count() == 1
            assert m.identify_languages(x) == first[1] and clf.predict(x) == [LABELS[i] for i in INTENDED]
            del junk
    assert m.selected_languages() == []
