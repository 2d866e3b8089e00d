"""The MMS language bank on the CPU: the open companion header include_open/thunder_speech_amd/mms_lang_bank.h through `_lib.OPEN` and the built
library's symbols; the bank's bookkeeping on a tiny random MMS config that never leaves the host (slot 0, add / load / remove / names, the id
buffer select_languages fills); and every refusal, by name and before any device work."""
import ctypes
import json
import math
import os
import subprocess

import pytest
import torch

transformers = pytest.importorskip("transformers")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, i32, f32, cint = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float, ctypes.c_int

NAMES = ["ts_mms_lang_bank_abi_version", "ts_mms_lang_bank_adapter_fwd", "ts_mms_lang_bank_head_fwd"]
SIGNATURES = {
    "ts_mms_lang_bank_abi_version": (cint, []),
    "ts_mms_lang_bank_adapter_fwd": (cint, [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, f32, vp, vp, i32, vp]),
    "ts_mms_lang_bank_head_fwd": (cint, [vp, i32, i32, i32, vp, vp, vp, i32, i32, vp, vp, i32, i32, vp]),
}

# the tiny MMS configuration and the two-language directory of tests/test_mms_host.py (copied: that file is not imported)
BASE = ["<pad>", "<s>", "</s>", "<unk>", "|"]
VOCABS = {"aaa": BASE + list("abcdefghijklmnopqrstuvwxyz'"), "bbb": BASE + list("zyxwvutsrq")}
CFG = dict(hidden_size=160, num_hidden_layers=2, num_attention_heads=2, intermediate_size=320, feat_extract_norm="layer", conv_bias=True,
           do_stable_layer_norm=True, vocab_size=len(VOCABS["aaa"]), conv_dim=(32,) * 7, conv_kernel=(10, 3, 3, 3, 3, 2, 2),
           conv_stride=(5, 2, 2, 2, 2, 2, 2), num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, pad_token_id=0, adapter_attn_dim=16)


# ---- the binder ------------------------------------------------------------------------------------------------------------------------------
def test_open_header_parses_and_declares_exactly_its_names():
    from thunder_speech_amd import _lib, build as b
    assert "mms_lang_bank" in _lib.OPEN
    h = _lib.OPEN["mms_lang_bank"]
    assert h.path == os.path.join(ROOT, "include_open", "thunder_speech_amd", "mms_lang_bank.h") and h.path in b.header_deps()
    assert list(h.signatures) == NAMES and h.signatures == SIGNATURES
    assert (h.version_define, h.version_function, h.abi_version) == ("TS_MMS_LANG_BANK_ABI_VERSION", "ts_mms_lang_bank_abi_version", 1)
    assert h.structs == {} and h.defines == {"TS_MMS_LANG_BANK_ABI_VERSION": 1}
    others = [o for o in (_lib.CORE, *_lib.COMPANIONS.values(), *_lib.STAGED.values(), *_lib.QUEUED.values(), *_lib.OPEN.values()) if o is not h]
    assert not set().union(*(o.signatures for o in others)) & set(NAMES)


def test_built_library_defines_the_names_and_reports_the_version():
    from thunder_speech_amd import build as b
    path = b.build(verbose=False)
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert not [n for n in NAMES if n not in defined]
    from thunder_speech_amd import _lib
    assert _lib.lib().ts_mms_lang_bank_abi_version() == 1          # host code: needs no GPU


# ---- a tiny MMS module on the host -----------------------------------------------------------------------------------------------------------
def _random_mms_ctc(seed, **kw):
    """tests/test_gpu_mms.py's: biases 0.1 randn everywhere, adapters with a non-trivial norm affine and a linear_2 of the order of the stream."""
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


class _Tok:
    """The two things text_transform_from_tokenizer reads of a tokenizer."""
    pad_token, unk_token, additional_special_tokens = "<pad>", "<unk>", []

    def __init__(self, tokens):
        self.tokens = tokens

    def get_vocab(self):
        return {t: i for i, t in enumerate(self.tokens)}


def _module(lang="aaa", precision="bf16", seed=3, **kw):
    from thunder_speech_amd.huggingface.compatibility import module_from_huggingface
    model = _random_mms_ctc(seed, vocab_size=len(VOCABS[lang]), **kw)
    m = module_from_huggingface(model, transformers.Wav2Vec2FeatureExtractor(return_attention_mask=True), _Tok(VOCABS[lang]))
    m.encoder.precision = precision
    return model, m


def _pack(lang, seed):
    """A language pack: the keys of _get_adapters() with random values."""
    shapes = _random_mms_ctc(seed, vocab_size=len(VOCABS[lang]))._get_adapters()
    g = torch.Generator().manual_seed(seed)
    return {k: torch.randn(v.shape, generator=g) for k, v in shapes.items()}


def _two_language_checkpoint(d):
    """tests/test_mms_host.py's: the model saved with the first language's head, adapter.<lang>.safetensors per language, a nested vocab.json."""
    from safetensors.torch import save_file
    torch.manual_seed(21)
    transformers.Wav2Vec2ForCTC(transformers.Wav2Vec2Config(**CFG)).eval().save_pretrained(d)
    adapters = {}
    for lang, toks in VOCABS.items():
        shapes = transformers.Wav2Vec2ForCTC(transformers.Wav2Vec2Config(**{**CFG, "vocab_size": len(toks)}))._get_adapters()
        adapters[lang] = {k: torch.randn_like(v).contiguous() for k, v in shapes.items()}
        save_file(adapters[lang], os.path.join(d, f"adapter.{lang}.safetensors"))
    with open(os.path.join(d, "vocab.json"), "w") as f:
        json.dump({lang: {tok: i for i, tok in enumerate(toks)} for lang, toks in VOCABS.items()}, f)
    transformers.Wav2Vec2CTCTokenizer(os.path.join(d, "vocab.json"), target_lang="aaa").save_pretrained(d)
    transformers.Wav2Vec2FeatureExtractor(return_attention_mask=True).save_pretrained(d)
    return adapters


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_slot_0_holds_the_resident_language_and_add_remove_write_in_place(precision):
    from thunder_speech_amd.huggingface.encoder import LORA_BANK_MAX_CLIPS
    model, m = _module(precision=precision)
    keys_before = list(m.state_dict())
    epoch = getattr(m.encoder, "_param_epoch", 0)
    m.language_bank("aaa", capacity=3)
    bank = m.__dict__["_language_bank"]
    assert m.encoder.__dict__["_language_bank"] is bank and m.encoder._param_epoch == epoch + 1
    assert list(m.state_dict()) == keys_before                     # plain tensors: no Parameters, no buffers
    dt = torch.bfloat16 if precision == "bf16" else torch.float32
    n = len(VOCABS["aaa"])
    assert bank.v_pad == 32 and bank.head_w.shape == (3, 32, 160) and bank.head_w.dtype == dt and bank.head_b.dtype == torch.float32
    assert bank.w1.shape == (2, 3, 16, 160) and bank.w2.shape == (2, 3, 160, 16) and bank.w1.dtype == dt and bank.norm_w.dtype == torch.float32
    assert bank.ids.shape == (LORA_BANK_MAX_CLIPS,) and bank.ids.dtype == torch.int32 and bool((bank.ids == -1).all())
    assert m.language_bank_names() == ["aaa"] and m.selected_languages() == [] and bank.vocab.tolist() == [n, 0, 0]
    sd = model.state_dict()
    for i in range(2):
        q = f"wav2vec2.encoder.layers.{i}.adapter_layer."
        assert torch.equal(bank.w1[i, 0], sd[q + "linear_1.weight"].to(dt)) and torch.equal(bank.w2[i, 0], sd[q + "linear_2.weight"].to(dt))
        assert torch.equal(bank.norm_w[i, 0], sd[q + "norm.weight"]) and torch.equal(bank.norm_b[i, 0], sd[q + "norm.bias"])
        assert torch.equal(bank.b1[i, 0], sd[q + "linear_1.bias"]) and torch.equal(bank.b2[i, 0], sd[q + "linear_2.bias"])
    assert torch.equal(bank.head_w[0, :n], sd["lm_head.weight"].to(dt)) and torch.equal(bank.head_b[0, :n], sd["lm_head.bias"])
    assert not bool(bank.head_w[0, n:].any()) and not bool(bank.head_b[0, n:].any())
    assert bank.transforms[0] is m.text_transform

    addresses = [getattr(bank, t).data_ptr() for t in bank._TENSORS]
    pack = _pack("bbb", 7)
    nb = len(VOCABS["bbb"])
    assert m.language_bank_add("bbb", pack, VOCABS["bbb"]) == 1
    assert m.language_bank_names() == ["aaa", "bbb"] and bank.vocab.tolist() == [n, nb, 0]
    assert torch.equal(bank.w2[1, 1], pack["wav2vec2.encoder.layers.1.adapter_layer.linear_2.weight"].to(dt))
    assert torch.equal(bank.head_w[1, :nb], pack["lm_head.weight"].to(dt)) and not bool(bank.head_w[1, nb:].any())
    tr = bank.transforms[1]
    assert list(tr.vocab.itos) == [" " if t == "|" else t for t in VOCABS["bbb"]] and tr.vocab.blank_idx == m.text_transform.vocab.blank_idx
    assert m.language_bank_add("ccc", _pack("bbb", 8), VOCABS["bbb"]) == 2
    m.select_languages(["bbb", None, "ccc", "aaa"])
    assert bank.ids[:6].tolist() == [1, -1, 2, 0, -1, -1] and bool((bank.ids[4:] == -1).all())
    assert m.selected_languages() == ["bbb", None, "ccc", "aaa"]
    m.language_bank_remove("bbb")                                  # its clips go back to the resident language; the slot is zeroed and free
    assert bank.ids[:4].tolist() == [-1, -1, 2, 0] and m.selected_languages() == [None, None, "ccc", "aaa"]
    assert m.language_bank_names() == ["aaa", "ccc"] and bank.vocab.tolist() == [n, 0, nb]
    assert not bool(bank.w1[:, 1].any()) and not bool(bank.head_w[1].any())
    assert m.language_bank_add("ddd", pack, VOCABS["bbb"]) == 1    # the freed slot
    assert [getattr(bank, t).data_ptr() for t in bank._TENSORS] == addresses


def test_language_bank_load_reads_a_two_language_directory(tmp_path):
    d = str(tmp_path / "mms")
    os.makedirs(d)
    adapters = _two_language_checkpoint(d)
    _, m = _module()
    m.language_bank("aaa", capacity=4)
    assert m.language_bank_load(d, ["bbb"]) == [1]
    bank = m.__dict__["_language_bank"]
    nb = len(VOCABS["bbb"])
    assert m.language_bank_names() == ["aaa", "bbb"] and bank.vocab.tolist()[:2] == [len(VOCABS["aaa"]), nb]
    assert torch.equal(bank.head_w[1, :nb], adapters["bbb"]["lm_head.weight"].to(torch.bfloat16))
    assert torch.equal(bank.w1[0, 1], adapters["bbb"]["wav2vec2.encoder.layers.0.adapter_layer.linear_1.weight"].to(torch.bfloat16))
    assert list(bank.transforms[1].vocab.itos) == [" " if t == "|" else t for t in VOCABS["bbb"]]
    with pytest.raises(KeyError, match="language_bank_load.*'zzz'"):
        m.language_bank_load(d, ["zzz"])


# ---- refusals, by name, before any device work --------------------------------------------------------------------------------------------
def test_language_bank_refuses_by_name():
    from thunder_speech_amd.huggingface.compatibility import module_from_huggingface
    plain = transformers.Wav2Vec2ForCTC(transformers.Wav2Vec2Config(**{**CFG, "adapter_attn_dim": None, "num_attention_heads": 4})).eval()
    m0 = module_from_huggingface(plain, transformers.Wav2Vec2FeatureExtractor(), _Tok(VOCABS["aaa"]))
    with pytest.raises(NotImplementedError, match="language_bank: the encoder has no attention adapters"):
        m0.language_bank("aaa")
    with pytest.raises(RuntimeError, match="select_languages: this module has no language bank"):
        m0.select_languages([])
    _, mx = _module()
    mx.encoder.__dict__["_precision"] = "mxfp8"                    # the mode refuses these checkpoints itself; the bank names it first
    with pytest.raises(NotImplementedError, match="language_bank: a language bank under precision='mxfp8'"):
        mx.language_bank("aaa")
    _, m = _module()
    with pytest.raises(ValueError, match="language_bank: max_vocab"):
        m.language_bank("aaa", max_vocab=16)                       # below the resident vocabulary
    with pytest.raises(ValueError, match="language_bank: max_vocab"):
        m.language_bank("aaa", max_vocab=40)                       # not a multiple of 16
    m.language_bank("aaa", capacity=2)
    with pytest.raises(RuntimeError, match="language_bank: this module already has a language bank"):
        m.language_bank("aaa")


def test_language_bank_add_select_and_remove_refuse_by_name():
    from thunder_speech_amd.huggingface.encoder import LORA_BANK_MAX_CLIPS
    _, m = _module()
    m.language_bank("aaa", capacity=2)
    pack = _pack("bbb", 7)
    with pytest.raises(RuntimeError, match="language_bank_add: the bank already holds a language named 'aaa'"):
        m.language_bank_add("aaa", pack, VOCABS["bbb"])
    missing = {k: v for k, v in pack.items() if k != "lm_head.bias"}
    with pytest.raises(KeyError, match="language_bank_add: keys differ"):
        m.language_bank_add("bbb", missing, VOCABS["bbb"])
    with pytest.raises(KeyError, match="language_bank_add: keys differ"):
        m.language_bank_add("bbb", {**pack, "wav2vec2.encoder.layers.2.adapter_layer.norm.bias": torch.zeros(160)}, VOCABS["bbb"])
    with pytest.raises(ValueError, match=r"language_bank_add: lm_head.weight has shape \(9, 160\)"):
        m.language_bank_add("bbb", {**pack, "lm_head.weight": torch.zeros(9, 160)}, VOCABS["bbb"])
    with pytest.raises(ValueError, match="language_bank_add: wav2vec2.encoder.layers.0.adapter_layer.linear_1.weight has shape"):
        m.language_bank_add("bbb", {**pack, "wav2vec2.encoder.layers.0.adapter_layer.linear_1.weight": torch.zeros(32, 160)}, VOCABS["bbb"])
    big = BASE + [chr(0x4E00 + i) for i in range(40)]               # 45 classes against max_vocab 32
    with pytest.raises(ValueError, match="language_bank_add: 'big' has a vocabulary of 45 classes, the bank was created with max_vocab=32"):
        m.language_bank_add("big", pack, big)
    moved = ["a", "<pad>"] + VOCABS["bbb"][2:]                      # the blank at index 1
    with pytest.raises(ValueError, match="language_bank_add: 'moved' has its blank '<pad>' at index 1, the resident language at 0"):
        m.language_bank_add("moved", pack, moved)
    assert m.language_bank_names() == ["aaa"]                       # nothing of the refused packs was written
    assert m.language_bank_add("bbb", pack, VOCABS["bbb"]) == 1
    with pytest.raises(RuntimeError, match="language_bank_add: the bank is full"):
        m.language_bank_add("ccc", pack, VOCABS["bbb"])
    with pytest.raises(KeyError, match="select_languages: no language named 'ccc'"):
        m.select_languages(["bbb", "ccc"])
    with pytest.raises(ValueError, match=f"select_languages: {LORA_BANK_MAX_CLIPS + 1} entries"):
        m.select_languages([None] * (LORA_BANK_MAX_CLIPS + 1))
    with pytest.raises(KeyError, match="language_bank_remove: no language named 'ccc'"):
        m.language_bank_remove("ccc")
    with pytest.raises(RuntimeError, match="language_bank_remove: 'aaa' is the resident language"):
        m.language_bank_remove("aaa")
    assert m.selected_languages() == [] and m.language_bank_names() == ["aaa", "bbb"]


def test_training_and_single_language_methods_are_refused_by_name_before_any_device_work():
    _, m = _module()
    m.language_bank("aaa", capacity=2)
    m.language_bank_add("bbb", _pack("bbb", 7), VOCABS["bbb"])
    x, n = torch.zeros(2, 4000), torch.tensor([4000, 4000])          # CPU tensors: every refusal comes before the GPU check
    m.train()
    with pytest.raises(NotImplementedError, match="training with a language bank is not implemented"):
        m(x, n)
    with pytest.raises(NotImplementedError, match="training with a language bank"):
        m.encoder(x, n)
    m.eval()
    m.select_languages(["bbb", None])
    for name, call in [("align", lambda: m.align(x, ["a", "b"])), ("predict_spans", lambda: m.predict_spans(x)),
                       ("predict_beam", lambda: m.predict_beam(x)), ("predict_nbest", lambda: m.predict_nbest(x, 2)),
                       ("logits_long", lambda: m.logits_long(x[0])), ("logits_long", lambda: m.transcribe_long(x[0])),
                       ("logits_long", lambda: m.predict_spans_long(x[0])), ("logits_long", lambda: m.align_long(x[0], ["a"]))]:
        with pytest.raises(NotImplementedError, match=f"{name}.*mixed selection of the language bank"):
            call()
    # under the all-resident selection (by name or by None) they go on to the GPU check as before
    m.select_languages(["aaa", None])
    with pytest.raises(RuntimeError, match="GPU tensors required") as e:
        m.align(x, ["a", "b"])
    assert not isinstance(e.value, NotImplementedError)
    with torch.no_grad(), pytest.raises(RuntimeError) as e:           # eval forward: the GPU check (no CPU path)
        m(x, n)
    assert not isinstance(e.value, NotImplementedError)


def test_predict_languages_restores_the_selection_when_predict_raises():
    _, m = _module()
    m.language_bank("aaa", capacity=2)
    m.language_bank_add("bbb", _pack("bbb", 7), VOCABS["bbb"])
    m.select_languages([None, "bbb"])
    bank = m.__dict__["_language_bank"]
    with torch.no_grad(), pytest.raises(RuntimeError):
        m.predict_languages(torch.zeros(2, 4000), ["bbb", "bbb"])      # CPU tensors: predict raises at the GPU check
    assert m.selected_languages() == [None, "bbb"] and bank.ids[:3].tolist() == [-1, 1, -1]
