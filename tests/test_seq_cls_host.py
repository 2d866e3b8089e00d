"""Audio classification heads on the CPU: the open companion header include_open/thunder_speech_amd/seq_cls.h through `_lib.OPEN` and the built
library's symbols and host-only entry points; the module classifier_from_huggingface assembles on tiny random transformers models that never
leave the host (state-dict keys, labels); the language router's class_slot table; and every refusal, by name and before any device work."""
import ctypes
import math
import os
import subprocess

import pytest
import torch

transformers = pytest.importorskip("transformers")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, i32, i64, f32, cint = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_int

NAMES = ["ts_seq_cls_abi_version", "ts_seq_cls_pool_launch_config", "ts_seq_cls_pool_workspace_bytes", "ts_seq_cls_pool",
         "ts_seq_cls_head_workspace_bytes", "ts_seq_cls_head"]
SIGNATURES = {
    "ts_seq_cls_abi_version": (cint, []),
    "ts_seq_cls_pool_launch_config": (cint, [i32, i32, vp, vp, vp]),
    "ts_seq_cls_pool_workspace_bytes": (i64, [i32, i32, i32]),
    "ts_seq_cls_pool": (cint, [vp, i32, i32, i32, vp, vp, i32, vp, vp]),
    "ts_seq_cls_head_workspace_bytes": (i64, [i32, i32]),
    "ts_seq_cls_head": (cint, [vp, i32, i32, i32, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, i32, vp]),
}
OUT_OF_SCOPE = ["Out of scope:", "fine-tuning classification heads", "ForAudioFrameClassification", "ForXVector", "sew-d",
                "relative-position conformers", "confidence threshold or fallback policy", "LM fusion, alignment and", "long-form transcription",
                "routed selection", "downloading checkpoints"]

# the tiny configurations of tests/test_gpu_family_finetune.py, test_gpu_wavlm.py, test_gpu_sew.py, test_gpu_conformer.py and of the MMS bank tests
# (copied: those files are not imported)
BASE = dict(vocab_size=32, hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128, conv_dim=(32, 32, 32),
            conv_stride=(5, 2, 2), conv_kernel=(10, 3, 2), num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4)
HD64 = dict(hidden_size=128, num_attention_heads=2, intermediate_size=256)
FAMILIES = {
    "wav2vec2": ("Wav2Vec2", dict(feat_extract_norm="group", do_stable_layer_norm=False)),
    "hubert": ("Hubert", dict(feat_extract_norm="group", do_stable_layer_norm=False)),
    "wavlm": ("WavLM", dict(HD64, feat_extract_norm="group", do_stable_layer_norm=False)),
    "sew": ("SEW", dict(HD64, conv_dim=(32, 32, 32, 32, 64), conv_kernel=(10, 3, 1, 3, 1), conv_stride=(5, 2, 1, 2, 1), squeeze_factor=2)),
    "conformer": ("Wav2Vec2Conformer", dict(HD64, position_embeddings_type="rotary", conv_depthwise_kernel_size=31)),
}
MMS_BASE = ["<pad>", "<s>", "</s>", "<unk>", "|"]
MMS_VOCABS = {"aaa": MMS_BASE + list("abcdefghijklmnopqrstuvwxyz'"), "bbb": MMS_BASE + list("zyxwvutsrq")}
MMS_CFG = dict(hidden_size=160, num_hidden_layers=2, num_attention_heads=2, intermediate_size=320, feat_extract_norm="layer", conv_bias=True,
               do_stable_layer_norm=True, vocab_size=len(MMS_VOCABS["aaa"]), conv_dim=(32,) * 7, conv_kernel=(10, 3, 3, 3, 3, 2, 2),
               conv_stride=(5, 2, 2, 2, 2, 2, 2), num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, pad_token_id=0, adapter_attn_dim=16)
LABELS = ["eng", "aaa", "fra", "bbb", "deu", "ccc"]


def _model(family, seed=0, **over):
    torch.manual_seed(seed)
    cls, kw = FAMILIES[family]
    cfg = getattr(transformers, cls + "Config")(**{**BASE, **kw, "classifier_proj_size": 32, "num_labels": 5, **over})
    return getattr(transformers, cls + "ForSequenceClassification")(cfg).eval()


def _classifier(family="wav2vec2", mask=False, **over):
    from thunder_speech_amd.huggingface import classifier_from_huggingface
    model = _model(family, **over)
    return model, classifier_from_huggingface(model, transformers.Wav2Vec2FeatureExtractor(return_attention_mask=mask))


# ---- the binder ------------------------------------------------------------------------------------------------------------------------------
def test_open_header_parses_and_declares_exactly_its_names():
    from thunder_speech_amd import _lib, build as b
    assert "seq_cls" in _lib.OPEN
    h = _lib.OPEN["seq_cls"]
    assert h.path == os.path.join(ROOT, "include_open", "thunder_speech_amd", "seq_cls.h") and h.path in b.header_deps()
    assert list(h.signatures) == NAMES and h.signatures == SIGNATURES
    assert (h.version_define, h.version_function, h.abi_version) == ("TS_SEQ_CLS_ABI_VERSION", "ts_seq_cls_abi_version", 1)
    assert h.structs == {} and h.defines == {"TS_SEQ_CLS_ABI_VERSION": 1}
    others = [o for o in (_lib.CORE, *_lib.COMPANIONS.values(), *_lib.STAGED.values(), *_lib.QUEUED.values(), *_lib.OPEN.values()) if o is not h]
    assert not set().union(*(o.signatures for o in others)) & set(NAMES)
    assert len(_lib.SIGNATURES) == 123 and _lib.ABI_VERSION == 15        # the core ABI is what it was


def test_header_names_what_is_out_of_scope_and_uses_mapped_types_only():
    with open(os.path.join(ROOT, "include_open", "thunder_speech_amd", "seq_cls.h")) as f:
        text = f.read()
    flat = " ".join(text.replace("*", " ").split())
    for phrase in OUT_OF_SCOPE:
        assert phrase in flat, phrase
    assert "divides by zero" in flat                                   # the len = 0 clip
    from thunder_speech_amd._lib import read_header
    import re
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    assert not re.search(r"\b(double|size_t)\b", code)
    read_header(text)                                                   # every type has a row: no error


def test_built_library_defines_the_names_and_reports_the_version():
    from thunder_speech_amd import build as b
    path = b.build(verbose=False)
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert not [n for n in NAMES if n not in defined]
    from thunder_speech_amd import _lib
    assert _lib.lib().ts_seq_cls_abi_version() == 1                     # host code: needs no GPU


def test_launch_config_and_workspace_sizes_depend_on_t_and_c_only():
    from thunder_speech_amd import _lib
    L = _lib.lib()

    def config(t, c):
        s, r, blk = i32(-1), i32(-1), i32(-1)
        assert L.ts_seq_cls_pool_launch_config(t, c, ctypes.byref(s), ctypes.byref(r), ctypes.byref(blk)) == 0
        return s.value, r.value, blk.value
    for t in (1, 31, 32, 33, 49, 130, 512, 513, 999, 3000, 100000):
        for c in (8, 160, 1280, 1288, 4096):
            s, r, blk = config(t, c)
            assert s >= 1 and r >= 1 and (s - 1) * r < t <= s * r       # the splits cover the t frames, none is empty
            assert s <= 16 and blk % 64 == 0 and 4 * blk >= c and blk <= 1024
            for batch in (1, 5, 16):
                assert L.ts_seq_cls_pool_workspace_bytes(batch, t, c) == 4 * batch * s * c
    assert config(1, 160)[0] == 1 and config(49, 160)[0] == 2 and config(130, 160)[0] == 5      # below, off and across the split
    assert config(999, 1280)[0] == 16                                   # 16 x 16 workgroups of 320 threads at the reference shape
    assert L.ts_seq_cls_pool_launch_config(130, 160, None, None, None) == 0
    assert L.ts_seq_cls_pool_launch_config(0, 160, None, None, None) == _lib.TS_EINVAL
    assert L.ts_seq_cls_pool_launch_config(130, 0, None, None, None) == _lib.TS_EINVAL
    assert L.ts_seq_cls_pool_launch_config(130, 164, None, None, None) == _lib.TS_EUNSUPPORTED
    assert L.ts_seq_cls_pool_launch_config(130, 4104, None, None, None) == _lib.TS_EUNSUPPORTED
    assert L.ts_seq_cls_pool_workspace_bytes(0, 130, 160) == 0 and L.ts_seq_cls_pool_workspace_bytes(65536, 130, 160) == 0
    assert L.ts_seq_cls_pool_workspace_bytes(4, 130, 164) == 0
    assert L.ts_seq_cls_head_workspace_bytes(5, 64) == 4 * 5 * 64
    assert L.ts_seq_cls_head_workspace_bytes(5, 72) == 0 and L.ts_seq_cls_head_workspace_bytes(5, 4112) == 0 and L.ts_seq_cls_head_workspace_bytes(0, 64) == 0


def test_argument_checks_return_before_any_launch():
    """Every TS_EINVAL / TS_EUNSUPPORTED of the header comes from host code in front of the launch: fake (aligned, never dereferenced) addresses."""
    from thunder_speech_amd import _lib
    L = _lib.lib()
    A, EI, EU = 0x10000, _lib.TS_EINVAL, _lib.TS_EUNSUPPORTED
    pool = lambda h=A, batch=2, t=49, c=160, ln=A, w=A, acc=0, out=A: L.ts_seq_cls_pool(h, batch, t, c, ln, w, acc, out, None)
    assert pool(h=None) == EI and pool(out=None) == EI and pool(batch=0) == EI and pool(t=0) == EI and pool(c=0) == EI
    assert pool(acc=2) == EI and pool(acc=-1) == EI
    assert pool(c=164) == EU and pool(c=4104) == EU and pool(batch=65536) == EU
    assert pool(h=A + 8) == EU and pool(out=A + 4) == EU and pool(ln=A + 2) == EU and pool(w=A + 1) == EU

    def head(partials=A, batch=2, t=49, c=160, pw=A, pb=A, p=64, cw=A, cb=A, n=12, cs=A, ws=A, logits=A, top1=A, logp=A, slot=A, prec=0):
        return L.ts_seq_cls_head(partials, batch, t, c, pw, pb, p, cw, cb, n, cs, ws, logits, top1, logp, slot, prec, None)
    for name in ("partials", "pw", "pb", "cw", "cb", "ws", "logits"):
        assert head(**{name: None}) == EI, name
    for name in ("batch", "t", "c", "p", "n"):
        assert head(**{name: 0}) == EI, name
    assert head(cs=None) == EI and head(slot=None) == EI               # one without the other
    assert head(c=164) == EU and head(c=4104) == EU and head(p=72) == EU and head(p=4112) == EU and head(n=8193) == EU
    assert head(batch=65536) == EU and head(prec=2) == EU and head(prec=-1) == EU
    for name in ("partials", "pw", "cw", "ws"):
        assert head(**{name: A + 8}) == EU, name
    for name in ("pb", "cb", "cs", "logits", "top1", "logp", "slot"):
        assert head(**{name: A + 2}) == EU, name


# ---- the module on the host ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("weighted", [False, True])
def test_module_keeps_transformers_state_dict_keys_and_labels_in_id_order(family, weighted):
    from thunder_speech_amd.huggingface.classification import AudioClassifierModule
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    from thunder_speech_amd.huggingface.transform import Wav2Vec2Preprocess
    if weighted and family in ("sew", "conformer"):
        with pytest.raises(NotImplementedError, match="use_weighted_layer_sum=True with model_type="):
            _classifier(family, use_weighted_layer_sum=True)
        return
    id2label = {3: "three", 0: "zero", 4: "four", 1: "one", 2: "two"}
    model, m = _classifier(family, mask=True, use_weighted_layer_sum=weighted, id2label=id2label, label2id={v: k for k, v in id2label.items()})
    assert isinstance(m, AudioClassifierModule) and not m.training
    assert isinstance(m.encoder, HuggingFaceEncoderAdapt) and m.encoder.original_encoder is model.base_model and m.encoder.mask_input
    assert isinstance(m.audio_transform, Wav2Vec2Preprocess) and m.audio_transform.mask_input and m.sample_rate == 16000
    assert m.labels == ["zero", "one", "two", "three", "four"]
    sd, ref = m.state_dict(), model.state_dict()
    head_keys = ["projector.weight", "projector.bias", "classifier.weight", "classifier.bias"] + (["layer_weights"] if weighted else [])
    assert sorted(k for k in sd if not k.startswith("encoder.")) == sorted(head_keys)
    for k in head_keys:
        assert sd[k].data_ptr() == ref[k].data_ptr()                    # transformers' own tensors under its own keys
    assert m.projector is model.projector and m.classifier is model.classifier
    assert (m.layer_weights is model.layer_weights) if weighted else (m.layer_weights is None)
    assert m.weighted_layer_sum == weighted


def test_labels_default_to_transformers_placeholder_names():
    _, m = _classifier(num_labels=3)
    assert m.labels == ["LABEL_0", "LABEL_1", "LABEL_2"]


def test_exports_and_loader_signature():
    import thunder_speech_amd.huggingface as hf
    from thunder_speech_amd.huggingface import classification as c
    assert hf.classifier_from_huggingface is c.classifier_from_huggingface and hf.load_huggingface_classifier is c.load_huggingface_classifier
    assert hf.AudioClassifierModule is c.AudioClassifierModule
    for phrase in ("Out of scope", "ForAudioFrameClassification", "ForXVector", "sew-d", "confidence threshold", "downloading checkpoints"):
        assert phrase in " ".join(c.__doc__.split())


def test_loader_reads_a_saved_directory(tmp_path):
    from thunder_speech_amd.huggingface import load_huggingface_classifier
    model = _model("wav2vec2", num_labels=4, id2label={i: s for i, s in enumerate("abcd")}, label2id={s: i for i, s in enumerate("abcd")})
    model.save_pretrained(str(tmp_path))
    transformers.Wav2Vec2FeatureExtractor(return_attention_mask=False).save_pretrained(str(tmp_path))
    m = load_huggingface_classifier(str(tmp_path))
    assert m.labels == list("abcd") and not m.encoder.mask_input
    assert torch.equal(m.state_dict()["classifier.weight"], model.state_dict()["classifier.weight"])


def test_refusals_arrive_by_name_before_the_gpu_check():
    x, n = torch.zeros(2, 4000), torch.tensor([4000, 4000])            # CPU tensors: every refusal comes before the GPU check
    with pytest.raises(NotImplementedError, match="model_type='sew-d'"):
        from thunder_speech_amd.huggingface import classifier_from_huggingface
        torch.manual_seed(0)
        sewd = transformers.SEWDForSequenceClassification(transformers.SEWDConfig(
            hidden_size=64, num_hidden_layers=1, num_attention_heads=4, intermediate_size=128, conv_dim=(32, 32, 32), conv_stride=(5, 2, 2),
            conv_kernel=(10, 3, 2), num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, classifier_proj_size=32, max_position_embeddings=64,
            position_buckets=16))
        classifier_from_huggingface(sewd, transformers.Wav2Vec2FeatureExtractor())
    with pytest.raises(NotImplementedError, match="wav2vec2-conformer HIP path: unsupported configuration"):
        _classifier("conformer", position_embeddings_type="relative")
    with pytest.raises(NotImplementedError, match=r"classifier_proj_size=24 \(the head kernel takes a multiple of 16 up to 4096\)"):
        _classifier(classifier_proj_size=24)
    with pytest.raises(NotImplementedError, match=r"classifier_proj_size=4112"):
        _classifier(classifier_proj_size=4112)
    with pytest.raises(NotImplementedError, match=r"num_labels=8193 \(the head kernel takes 1 to 8192 classes\)"):
        _classifier(num_labels=8193)
    with pytest.raises(NotImplementedError, match="Wav2Vec2ForCTC has no `projector` Linear"):
        from thunder_speech_amd.huggingface import classifier_from_huggingface
        classifier_from_huggingface(transformers.Wav2Vec2ForCTC(transformers.Wav2Vec2Config(**{**BASE, **FAMILIES["wav2vec2"][1]})),
                                    transformers.Wav2Vec2FeatureExtractor())
    _, m = _classifier(use_weighted_layer_sum=True)
    m.train()
    with pytest.raises(NotImplementedError, match="audio classification: training mode is not implemented"):
        m(x, n)
    with pytest.raises(NotImplementedError, match="training mode"):
        m.predict(x)
    m.eval()
    m.encoder.__dict__["_precision"] = "mxfp8"
    with pytest.raises(NotImplementedError, match="use_weighted_layer_sum under precision='mxfp8'"):
        m.predict_topk(x, 2)
    m.encoder.__dict__["_precision"] = "bf16"
    with torch.no_grad(), pytest.raises(RuntimeError, match="MI355X only") as e:        # eval forward: the GPU check (no CPU path)
        m(x, n)
    assert not isinstance(e.value, NotImplementedError)


# ---- the router's table ------------------------------------------------------------------------------------------------------------------------
class _Tok:
    """The two things text_transform_from_tokenizer reads of a tokenizer."""
    pad_token, unk_token, additional_special_tokens = "<pad>", "<unk>", []

    def __init__(self, tokens):
        self.tokens = tokens

    def get_vocab(self):
        return {t: i for i, t in enumerate(self.tokens)}


def _mms_module(seed=3):
    from thunder_speech_amd.huggingface.compatibility import module_from_huggingface
    torch.manual_seed(seed)
    model = transformers.Wav2Vec2ForCTC(transformers.Wav2Vec2Config(**MMS_CFG)).eval()
    return module_from_huggingface(model, transformers.Wav2Vec2FeatureExtractor(return_attention_mask=True), _Tok(MMS_VOCABS["aaa"]))


def _pack(lang, seed):
    torch.manual_seed(seed)
    shapes = transformers.Wav2Vec2ForCTC(transformers.Wav2Vec2Config(**{**MMS_CFG, "vocab_size": len(MMS_VOCABS[lang])}))._get_adapters()
    g = torch.Generator().manual_seed(seed)
    return {k: torch.randn(v.shape, generator=g) for k, v in shapes.items()}


def _lid(labels=LABELS, **over):
    return _classifier(num_labels=len(labels), id2label=dict(enumerate(labels)), label2id={s: i for i, s in enumerate(labels)}, **over)[1]


def test_class_slot_table_identity_and_explicit_mappings_rewritten_in_place():
    m, clf = _mms_module(), _lid()
    m.language_bank("aaa", capacity=3)
    m.language_router(clf)                                              # the identity: label "aaa" -> language "aaa"
    router = m.__dict__["_language_router"]
    table = router.class_slot
    assert table.dtype == torch.int32 and table.shape == (6,) and table.device == m.__dict__["_language_bank"].device
    assert table.tolist() == [-1, 0, -1, -1, -1, -1]                    # classes of absent languages: -1
    ptr = table.data_ptr()
    assert m.language_bank_add("bbb", _pack("bbb", 7), MMS_VOCABS["bbb"]) == 1
    assert router.class_slot.data_ptr() == ptr and table.tolist() == [-1, 0, -1, 1, -1, -1]
    assert m.language_bank_add("ccc", _pack("bbb", 8), MMS_VOCABS["bbb"]) == 2
    assert table.tolist() == [-1, 0, -1, 1, -1, 2]
    m.language_bank_remove("bbb")
    assert router.class_slot.data_ptr() == ptr and table.tolist() == [-1, 0, -1, -1, -1, 2]
    m.language_router(clf, {"eng": "aaa", "fra": "ccc", "deu": "zzz", "bbb": "bbb"})      # explicit: several labels, one absent language
    t2 = m.__dict__["_language_router"].class_slot
    assert t2.tolist() == [0, -1, 2, -1, -1, -1]
    assert m.language_bank_add("zzz", _pack("bbb", 9), MMS_VOCABS["bbb"]) == 1
    assert t2.tolist() == [0, -1, 2, -1, 1, -1]
    assert m.selected_languages() == [] and bool((m.__dict__["_language_bank"].ids == -1).all())


def test_router_refusals_by_name():
    m, clf = _mms_module(), _lid()
    with pytest.raises(RuntimeError, match="language_router: this module has no language bank"):
        m.language_router(clf)
    m.language_bank("aaa", capacity=2)
    x = torch.zeros(2, 4000)
    with pytest.raises(RuntimeError, match="predict_auto: this module has no language router"):
        m.predict_auto(x)
    with pytest.raises(RuntimeError, match="identify_languages: this module has no language router"):
        m.identify_languages(x)
    with pytest.raises(KeyError, match=r"language_router: the mapping names labels the classifier does not have: \['xxx'\]"):
        m.language_router(clf, {"eng": "aaa", "xxx": "aaa"})
    with pytest.raises(TypeError, match="language_router: the classifier must be an AudioClassifierModule"):
        m.language_router(m)
    clf.audio_transform.sample_rate = 8000
    with pytest.raises(ValueError, match="language_router: the classifier takes waveforms at 8000 Hz, the module at 16000 Hz"):
        m.language_router(clf)
    clf.audio_transform.sample_rate = 16000
    assert "_language_router" not in m.__dict__
    m.language_router(clf)
    clf.train()
    with pytest.raises(NotImplementedError, match="training mode"):
        m.predict_auto(x)
    clf.eval()
    m.train()
    with pytest.raises(NotImplementedError, match="training with a language bank"):
        m.identify_languages(x)
    m.eval()
    m.select_languages([None, "aaa"])
    with torch.no_grad(), pytest.raises(RuntimeError, match="MI355X only"):       # then the GPU check; the selection stands
        m.predict_auto(x)
    assert m.selected_languages() == [None, "aaa"]
