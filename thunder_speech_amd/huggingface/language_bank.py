"""Many MMS languages on one module (no reference counterpart; include_open/thunder_speech_amd/mms_lang_bank.h, csrc/mms_lang_bank.hip).

An MMS checkpoint is one frozen base plus a pack per language: the attention adapters of every layer and a CTC head on that language's
vocabulary.  `LanguageBank` holds `capacity` such packs as plain tensors at fixed addresses next to the one packed base; every clip of a batch
names its language through one id buffer that the kernels read at run time.  Adding, removing and selecting write in place, so a captured
graph keeps serving whatever the mix of languages in the batch.  The public surface is BaseCTCModule's (language_bank, language_bank_add,
language_bank_load, language_bank_remove, language_bank_names, select_languages, selected_languages, predict_languages); the module owns the
head and the text transforms, the encoder's plan reads the adapters (Wav2Vec2Plan._attn_adapter), both through the bank's `ids`.

Who fills in the ids: `language_router` attaches an audio classifier (huggingface/classification.py: the MMS language-identification checkpoints)
whose head writes every clip's slot into `ids` on the device (ts_seq_cls_head's `slot` output), so `predict_auto` replays ONE graph -- classifier,
then ASR -- with no host work in between.  Out of scope: a confidence threshold or fallback policy for the router; LM fusion, alignment and
long-form transcription under a routed selection (refused as under any mixed selection)."""
from __future__ import annotations

import json
import os
from typing import Dict, List, Optional, Sequence

import torch

from .. import _lib
from ..text_processing.transform import BatchTextTransformer
from .encoder import LORA_BANK_MAX_CLIPS, HuggingFaceEncoderAdapt, has_attn_adapters

__all__ = ["LanguageBank"]

ADAPTER_TENSORS = ("norm.weight", "norm.bias", "linear_1.weight", "linear_1.bias", "linear_2.weight", "linear_2.bias")
HEAD_MAX_VOCAB = 4096              # ts_mms_lang_bank_head_fwd: v_pad a multiple of 16 up to 4096


def _round_up(n: int, m: int) -> int:
    return -(-int(n) // m) * m


class LanguageBank:
    """The tensors of BaseCTCModule.language_bank().  Per layer the six adapter tensors as [layers][capacity][...]: norm_w, norm_b [c], w1 [a][c],
    b1 [a], w2 [c][a], b2 [c] -- w1 / w2 in the GEMM operands' dtype (bf16 under precision="bf16", f32 under "fp32"), the rest f32; the heads
    head_w [capacity][v_pad][c] (operand dtype) and head_b [capacity][v_pad] (f32), zero beyond a language's vocabulary; vocab int32 [capacity]: the
    classes of the language in the slot; ids int32 [LORA_BANK_MAX_CLIPS]: the slot of clip b, -1 = the resident language (slot 0).  Host side: the
    slots' names and one text transform per slot."""

    _TENSORS = ("norm_w", "norm_b", "w1", "b1", "w2", "b2", "head_w", "head_b", "vocab", "ids")

    def __init__(self, n_layers: int, hidden: int, adapter_dim: int, capacity: int, v_pad: int, precision: str, device):
        self.n_layers, self.hidden, self.adapter_dim, self.capacity, self.v_pad, self.precision = n_layers, hidden, adapter_dim, capacity, v_pad, precision
        self.dtype = torch.float32 if precision == "fp32" else torch.bfloat16
        c, a = hidden, adapter_dim
        z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=device)
        self.norm_w, self.norm_b, self.b2 = z(n_layers, capacity, c), z(n_layers, capacity, c), z(n_layers, capacity, c)
        self.b1 = z(n_layers, capacity, a)
        self.w1, self.w2 = z(n_layers, capacity, a, c, dtype=self.dtype), z(n_layers, capacity, c, a, dtype=self.dtype)
        self.head_w, self.head_b = z(capacity, v_pad, c, dtype=self.dtype), z(capacity, v_pad)
        self.vocab = z(capacity, dtype=torch.int32)
        self.ids = torch.full((LORA_BANK_MAX_CLIPS,), -1, dtype=torch.int32, device=device)
        self.names: List[Optional[str]] = [None] * capacity        # slot -> language
        self.transforms: List[Optional[BatchTextTransformer]] = [None] * capacity
        self.selection: List[Optional[str]] = []                    # what select_languages() was last given: a language or None per clip

    @property
    def device(self):
        return self.ids.device

    def to(self, device) -> None:
        """Move the tensors (new addresses: the caller retires the graphs captured on the old ones)."""
        for name in self._TENSORS:
            setattr(self, name, getattr(self, name).to(device))

    def adapter_shapes(self, prefix: str) -> Dict[str, tuple]:
        """{key: shape} of a language pack, the keys of transformers' `model._get_adapters()` without the head (`prefix`: "wav2vec2.")."""
        c, a = self.hidden, self.adapter_dim
        shape = dict(zip(ADAPTER_TENSORS, ((c,), (c,), (a, c), (a,), (c, a), (c,))))
        return {f"{prefix}encoder.layers.{i}.adapter_layer.{k}": shape[k] for i in range(self.n_layers) for k in ADAPTER_TENSORS}

    def write_slot(self, slot: int, name: str, adapters: Sequence[torch.Tensor], head_w: torch.Tensor, head_b: torch.Tensor,
                   transform: BatchTextTransformer) -> None:
        """A language into `slot`, in place.  adapters: the six tensors of layer 0, then of layer 1, ... in ADAPTER_TENSORS order."""
        n = int(head_w.shape[0])
        with torch.no_grad():
            for i in range(self.n_layers):
                for dst, src in zip((self.norm_w, self.norm_b, self.w1, self.b1, self.w2, self.b2), adapters[6 * i: 6 * i + 6]):
                    dst[i, slot].copy_(src.detach().to(torch.float32))        # the operand dtype's rounding is the plan's: f32 -> bf16, nearest even
            self.head_w[slot].zero_()
            self.head_b[slot].zero_()
            self.head_w[slot, :n].copy_(head_w.detach().to(torch.float32))
            self.head_b[slot, :n].copy_(head_b.detach().to(torch.float32))
            self.vocab[slot: slot + 1].copy_(torch.tensor([n], dtype=torch.int32))
        self.names[slot], self.transforms[slot] = name, transform

    def clear_slot(self, slot: int) -> None:
        with torch.no_grad():
            for t in (self.norm_w, self.norm_b, self.w1, self.b1, self.w2, self.b2):
                t[:, slot].zero_()
            self.head_w[slot].zero_()
            self.head_b[slot].zero_()
            self.vocab[slot: slot + 1].zero_()
        self.names[slot], self.transforms[slot] = None, None

    def slots(self, n_clips: int) -> List[int]:
        """The slot that serves each of the first `n_clips` clips under the current selection (host side)."""
        sel = self.selection[:n_clips] + [None] * max(0, n_clips - len(self.selection))
        return [0 if name is None else self.names.index(name) for name in sel]

    def mixed(self) -> bool:
        """Does any clip select a language other than the resident one?"""
        return any(name is not None and name != self.names[0] for name in self.selection)

    def write_ids(self) -> None:
        """The id buffer from `selection`: the slots of the given clips, -1 for a None and for every entry beyond them.  One host-to-device copy at
        a fixed address."""
        host = torch.full((LORA_BANK_MAX_CLIPS,), -1, dtype=torch.int32)
        for i, name in enumerate(self.selection):
            if name is not None:
                host[i] = self.names.index(name)
        self.ids.copy_(host)

    # ---- the two launches ---------------------------------------------------------------------------------------------------------------
    def adapter(self, L, stream, h: torch.Tensor, layer: int, next_ln, eps: float, y, y_op, prec: int) -> None:
        """ts_mms_lang_bank_adapter_fwd on the residual stream h [b][t][c] with layer `layer`'s banks (Wav2Vec2Plan._attn_adapter)."""
        b, t, c = h.shape
        ptr = lambda x: x.data_ptr() if x is not None else None
        st = L.ts_mms_lang_bank_adapter_fwd(h.data_ptr(), b, t, c, self.adapter_dim, self.norm_w[layer].data_ptr(), self.norm_b[layer].data_ptr(),
                                            self.w1[layer].data_ptr(), self.b1[layer].data_ptr(), self.w2[layer].data_ptr(), self.b2[layer].data_ptr(),
                                            self.capacity, self.ids.data_ptr(), next_ln[0].data_ptr(), next_ln[1].data_ptr(), eps, ptr(y), ptr(y_op),
                                            prec, stream)
        _lib.check(st, "ts_mms_lang_bank_adapter_fwd")

    def head(self, h: torch.Tensor) -> torch.Tensor:
        """Logits [B, v_pad, T] (a view of a [B, v_pad, round_up(T, 4)] buffer) of the time-major encoder output h [B, T, C]: every clip with the
        head of its language, the classes beyond that language's vocabulary at -1e30."""
        if h.dtype != torch.float32 or not h.is_contiguous():
            h = h.to(torch.float32).contiguous()
        b, t, c = h.shape
        ldt = _round_up(t, 4)
        logits = torch.empty(b, self.v_pad, ldt, dtype=torch.float32, device=h.device)
        st = _lib.lib().ts_mms_lang_bank_head_fwd(h.data_ptr(), b, t, c, self.head_w.data_ptr(), self.head_b.data_ptr(), self.vocab.data_ptr(),
                                                  self.capacity, self.v_pad, self.ids.data_ptr(), logits.data_ptr(), ldt,
                                                  0 if self.precision == "fp32" else 1, torch.cuda.current_stream(h.device).cuda_stream)
        _lib.check(st, "ts_mms_lang_bank_head_fwd")
        return logits[:, :, :t]


# ---- what BaseCTCModule's methods do (module.py keeps the signatures and docstrings) --------------------------------------------------------
def _bank(module, what: str) -> LanguageBank:
    bank = module.__dict__.get("_language_bank")
    if bank is None:
        raise RuntimeError(f"{what}: this module has no language bank (language_bank() creates one)")
    return bank


def _transform_for(resident: BatchTextTransformer, tokens: Sequence[str]) -> BatchTextTransformer:
    """The text transform of a token list in id order, built as compatibility.text_transform_from_tokenizer builds the module's own: the word
    delimiter "|" shown as a space, the special tokens those of the resident language's tokenizer."""
    v = resident.vocab
    return BatchTextTransformer(tokens=[" " if t == "|" else str(t) for t in tokens], blank_token=v.blank_token, pad_token=v.pad_token,
                                unknown_token=v.unknown_token)


def create(module, name: str, capacity: int = 8, max_vocab: Optional[int] = None) -> None:
    enc = module.encoder
    if not isinstance(enc, HuggingFaceEncoderAdapt) or not has_attn_adapters(enc.original_encoder.config):
        raise NotImplementedError("language_bank: the encoder has no attention adapters (an MMS checkpoint, config.adapter_attn_dim, has them); "
                                  "banks on the conformer, SEW and WavLM plans are not implemented")
    if enc.precision == "mxfp8":
        raise NotImplementedError("language_bank: a language bank under precision='mxfp8' is not implemented; use precision='bf16' or 'fp32'")
    if module.__dict__.get("_language_bank") is not None:
        raise RuntimeError("language_bank: this module already has a language bank (one bank per module; language_bank_add() fills its slots)")
    if not isinstance(name, str) or not name:
        raise ValueError(f"language_bank: the resident language's name must be a non-empty string, got {name!r}")
    if isinstance(capacity, bool) or not isinstance(capacity, int) or capacity < 1:
        raise ValueError(f"language_bank: capacity must be a positive number of slots, got {capacity!r}")
    if module.decoder is None or module.text_transform is None:
        raise RuntimeError("language_bank: the module has no CTC head or text transform (the checkpoint came without a tokenizer)")
    head = module.decoder[2]
    n = int(head.weight.shape[0])
    v_pad = _round_up(n, 16) if max_vocab is None else int(max_vocab)
    if v_pad < n or v_pad % 16 or v_pad > HEAD_MAX_VOCAB:
        raise ValueError(f"language_bank: max_vocab must be a multiple of 16 from the resident vocabulary's {n} classes up to {HEAD_MAX_VOCAB}, "
                         f"got {max_vocab!r}")
    cfg = enc.original_encoder.config
    device = next(enc.original_encoder.parameters()).device
    plan = enc._plan(device)
    sd = enc.original_encoder.state_dict()
    bank = LanguageBank(int(cfg.num_hidden_layers), int(cfg.hidden_size), int(cfg.adapter_attn_dim), capacity, v_pad, enc.precision, device)
    bank.write_slot(0, name, [sd[k] for k in plan.attn_adapter_keys], head.weight, head.bias, module.text_transform)
    module.__dict__["_language_bank"] = enc.__dict__["_language_bank"] = bank
    enc._param_epoch = getattr(enc, "_param_epoch", 0) + 1        # graphs of the bank-less launch sequence are retired


def add(module, lang: str, adapter_sd: Dict[str, torch.Tensor], tokens: Sequence[str]) -> int:
    bank = _bank(module, "language_bank_add")
    if not isinstance(lang, str) or not lang:
        raise ValueError(f"language_bank_add: the language must be a non-empty string, got {lang!r}")
    if lang in bank.names:
        raise RuntimeError(f"language_bank_add: the bank already holds a language named {lang!r} (language_bank_remove() it first)")
    if None not in bank.names:
        raise RuntimeError(f"language_bank_add: the bank is full ({bank.capacity} slots: {', '.join(bank.names)}); language_bank_remove() frees one")
    tokens = list(tokens)
    n = len(tokens)
    if n > bank.v_pad:
        raise ValueError(f"language_bank_add: {lang!r} has a vocabulary of {n} classes, the bank was created with max_vocab={bank.v_pad}")
    prefix = getattr(module.encoder.original_encoder, "base_model_prefix", "wav2vec2") + "."
    want = bank.adapter_shapes(prefix)
    want.update({"lm_head.weight": (n, bank.hidden), "lm_head.bias": (n,)})
    if set(adapter_sd) != set(want):
        raise KeyError(f"language_bank_add: keys differ (missing {sorted(set(want) - set(adapter_sd))[:3]}, "
                       f"unexpected {sorted(set(adapter_sd) - set(want))[:3]})")
    for k, shape in want.items():
        if tuple(adapter_sd[k].shape) != shape:
            raise ValueError(f"language_bank_add: {k} has shape {tuple(adapter_sd[k].shape)}, expected {shape}")
    transform = _transform_for(bank.transforms[0], tokens)
    blank = bank.transforms[0].vocab.blank_idx
    if len(transform.vocab.itos) != n or transform.vocab.blank_idx != blank:
        raise ValueError(f"language_bank_add: {lang!r} has its blank {transform.vocab.blank_token!r} at index "
                         f"{transform.vocab.blank_idx if len(transform.vocab.itos) == n else None}, the resident language at {blank}; the greedy "
                         "decode of a batch has one blank index")
    slot = bank.names.index(None)
    bank.write_slot(slot, lang, [adapter_sd[k] for k in want if k.startswith(prefix)], adapter_sd["lm_head.weight"], adapter_sd["lm_head.bias"],
                    transform)
    _rewrite_router(module)                                         # the classes mapped to `lang` route to its slot from now on
    return slot


def load(module, model_dir: str, langs: Sequence[str]) -> List[int]:
    from safetensors.torch import load_file
    _bank(module, "language_bank_load")
    with open(os.path.join(model_dir, "vocab.json")) as f:
        vocab = json.load(f)
    slots = []
    for lang in [langs] if isinstance(langs, str) else list(langs):
        path = os.path.join(model_dir, f"adapter.{lang}.safetensors")
        if lang not in vocab or not isinstance(vocab[lang], dict) or not os.path.exists(path):
            raise KeyError(f"language_bank_load: {model_dir} has no language {lang!r} (it needs adapter.{lang}.safetensors and that entry of the nested vocab.json)")
        tokens = [tok for tok, _ in sorted(vocab[lang].items(), key=lambda kv: kv[1])]
        slots.append(add(module, lang, load_file(path), tokens))
    return slots


def remove(module, lang: str) -> None:
    bank = _bank(module, "language_bank_remove")
    if lang not in bank.names or lang is None:
        raise KeyError(f"language_bank_remove: no language named {lang!r} in the bank (it holds: {', '.join(names(module))})")
    slot = bank.names.index(lang)
    if slot == 0:
        raise RuntimeError(f"language_bank_remove: {lang!r} is the resident language (slot 0: every id outside the bank is served by it); it cannot be removed")
    if lang in bank.selection:
        bank.selection = [None if n == lang else n for n in bank.selection]
        bank.write_ids()
    bank.clear_slot(slot)
    _rewrite_router(module)                                         # the classes mapped to `lang` route to the resident language again


def names(module) -> List[str]:
    return [n for n in _bank(module, "language_bank_names").names if n is not None]


# ---- the router: an audio classifier fills in the ids (huggingface/classification.py, thunder_speech_amd/seq_cls.h) ---------------------------
class LanguageRouter:
    """An AudioClassifierModule next to a bank: `mapping` {classifier label: bank language}; class_slot int32 [n_labels] on the bank's device:
    the slot of the language a class is mapped to, -1 for a class of a language the bank does not hold (or of no language).  The table is
    rewritten IN PLACE whenever the bank's languages change, so a captured graph routes to a language added after its capture."""

    def __init__(self, classifier, mapping: Dict[str, str], bank: LanguageBank):
        self.classifier, self.mapping = classifier, dict(mapping)
        self.class_slot = torch.full((len(classifier.labels),), -1, dtype=torch.int32, device=bank.device)
        self.scratch = torch.full((LORA_BANK_MAX_CLIPS,), -1, dtype=torch.int32, device=bank.device)      # identify_languages' slots
        self.rewrite(bank)

    def rewrite(self, bank: LanguageBank) -> None:
        host = torch.full((len(self.classifier.labels),), -1, dtype=torch.int32)
        for i, label in enumerate(self.classifier.labels):
            lang = self.mapping.get(label)
            if lang is not None and lang in bank.names:
                host[i] = bank.names.index(lang)
        if self.class_slot.device != bank.device:                   # the bank moved: new addresses (the auto graphs are retired by the epoch)
            self.class_slot, self.scratch = self.class_slot.to(bank.device), self.scratch.to(bank.device)
        self.class_slot.copy_(host)


def _rewrite_router(module) -> None:
    router = module.__dict__.get("_language_router")
    if router is not None:
        router.rewrite(module.__dict__["_language_bank"])


def _router(module, what: str) -> LanguageRouter:
    _bank(module, what)
    router = module.__dict__.get("_language_router")
    if router is None:
        raise RuntimeError(f"{what}: this module has no language router (language_router() attaches a classifier)")
    return router


def attach_router(module, classifier, mapping: Optional[Dict[str, str]] = None) -> None:
    bank = _bank(module, "language_router")
    from .classification import AudioClassifierModule
    if not isinstance(classifier, AudioClassifierModule):
        raise TypeError(f"language_router: the classifier must be an AudioClassifierModule, got {type(classifier).__name__}")
    if int(classifier.sample_rate) != int(module.sample_rate):
        raise ValueError(f"language_router: the classifier takes waveforms at {classifier.sample_rate} Hz, the module at {module.sample_rate} Hz; "
                         "both read the same batch")
    if mapping is None:
        mapping = {label: label for label in classifier.labels}
    else:
        unknown = [k for k in mapping if k not in classifier.labels]
        if unknown:
            raise KeyError(f"language_router: the mapping names labels the classifier does not have: {unknown[:5]} (it has {len(classifier.labels)}: "
                           f"{', '.join(classifier.labels[:5])}, ...)")
        bad = [(k, v) for k, v in mapping.items() if not isinstance(v, str) or not v]
        if bad:
            raise ValueError(f"language_router: the mapping's languages must be non-empty strings, got {bad[:3]}")
    module.__dict__["_language_router"] = LanguageRouter(classifier, mapping, bank)
    module.__dict__.pop("_auto_graphs", None)


def _check_auto(module, what: str, x: torch.Tensor):
    """(bank, router) of a routed forward of the batch `x`; the refusals by name, before any device work."""
    router = _router(module, what)
    bank = check_forward(module, x)
    router.classifier._check_forward()
    return bank, router


def identify(module, x: torch.Tensor) -> List[Optional[str]]:
    bank, router = _check_auto(module, "identify_languages", x)
    clf = router.classifier
    if router.class_slot.device != bank.device:
        router.rewrite(bank)
    b = int(x.shape[0])
    xx = clf._prepare(x)
    lengths = torch.full((b,), x.shape[-1], dtype=torch.int32, device=xx.device)
    with torch.no_grad():
        clf._run(xx, lengths, class_slot=router.class_slot, slot=router.scratch)
    return [bank.names[s] if 0 <= s < bank.capacity else None for s in router.scratch[:b].tolist()]


def auto_forward(module, x: torch.Tensor):
    """One replay of the routed graph of x's signature (captured on first use): the classifier's front end, encoder, pool and head -- the head
    writes every clip's slot into bank.ids[:B] -- then the module's front end, encoder with the bank's adapters, ts_mms_lang_bank_head_fwd and
    the greedy decode; no host work between the two encoders.  -> (logits, output lengths, packed): the graph's OWN buffers; packed int32 =
    collapsed [B * T'], counts [B], ids [B] for one device-to-host read.  The bank's id buffer holds the ROUTED slots afterwards: the caller
    restores the selection (bank.write_ids())."""
    from ..module import greedy_decode
    from ..utils import GraphedForward
    bank, router = _check_auto(module, "predict_auto", x)
    clf = router.classifier
    if router.class_slot.device != bank.device:
        router.rewrite(bank)
    xx = clf._prepare(x)                                            # refreshes the head's operands and the soft-maxed layer weights
    b = int(xx.shape[0])
    lengths = torch.full((b,), xx.shape[-1], dtype=torch.int32, device=xx.device)

    def run(x_in, ll):
        clf._run(x_in, ll, class_slot=router.class_slot, slot=bank.ids)
        logits, out_lengths = module._forward_eager(x_in, ll)
        _, collapsed, counts = greedy_decode(logits)
        return logits, out_lengths, torch.cat((collapsed.reshape(-1), counts.reshape(-1), bank.ids[:b]))

    if torch.cuda.is_current_stream_capturing():                    # the caller records its own graph: launch into it
        with torch.no_grad():
            return run(xx, lengths)
    # a table of its own: _graphed_inference and its stamp stay as they are.  The stamp covers both modules' weights and the classifier's
    # device operands (operand_epoch moves whenever _refresh, called by _prepare above, allocated the head's operands or the soft-max buffer
    # anew -- after clf.eval() or clf.to(), which change no parameter); the bank's tensors, the class_slot table and the soft-maxed layer
    # weights are written in place and retire nothing
    stamp = (module._weights_stamp(), clf._weights_stamp() - clf._layer_weights_version(), clf.encoder.precision, clf.operand_epoch, id(router),
             router.class_slot.data_ptr(), bank.ids.data_ptr())
    graphs = module.__dict__.get("_auto_graphs")
    if graphs is None or graphs[0] != stamp:
        # recorded on the module's capture stream, as _graphed_inference's graphs: the launch arena is keyed by stream
        streams = module.__dict__.setdefault("_infer_streams", {})
        side = streams.get(str(xx.device))
        if side is None:
            side = streams[str(xx.device)] = torch.cuda.Stream(device=xx.device)
        graphs = module.__dict__["_auto_graphs"] = (stamp, GraphedForward(run, stream=side))
    return graphs[1](xx, lengths)


def predict_auto(module, x: torch.Tensor):
    bank = module.__dict__.get("_language_bank")                   # auto_forward makes the checks, by name, before any device work
    try:
        with torch.no_grad():
            logits, _, packed = auto_forward(module, x)
        b, t = int(logits.shape[0]), int(logits.shape[2])
        host = packed.to("cpu")                                     # the one device-to-host read
    finally:
        if bank is not None:
            bank.write_ids()                                        # the selection of select_languages holds again
    collapsed, counts, ids = host[: b * t].view(b, t), host[b * t: b * t + b], host[b * t + b:].tolist()
    slots = [s if 0 <= s < bank.capacity and bank.names[s] is not None else 0 for s in ids]
    texts: List[Optional[str]] = [None] * b
    for s in sorted(set(slots)):
        idx = [i for i, si in enumerate(slots) if si == s]
        for i, text in zip(idx, bank.transforms[s].decode_collapsed(collapsed[idx], counts[idx])):
            texts[i] = text
    return texts, [bank.names[s] for s in slots]


def select(module, langs) -> None:
    bank = _bank(module, "select_languages")
    langs = list(langs)
    if len(langs) > LORA_BANK_MAX_CLIPS:
        raise ValueError(f"select_languages: {len(langs)} entries; the bank's id buffer holds {LORA_BANK_MAX_CLIPS} clips")
    for n in langs:
        if n is not None and n not in bank.names:
            raise KeyError(f"select_languages: no language named {n!r} in the bank (it holds: {', '.join(names(module))})")
    bank.selection = langs
    bank.write_ids()


def refuse_mixed(module, what: str) -> None:
    """`what` turns text into ids, or carries an LM, of ONE language: refused while any clip selects a non-resident language."""
    bank = module.__dict__.get("_language_bank")
    if bank is not None and bank.mixed():
        raise NotImplementedError(f"{what}: not implemented under a mixed selection of the language bank (selected: {bank.selection}; the method "
                                  f"works with one vocabulary, the resident language {bank.names[0]!r}'s); select_languages([]) first")


def check_forward(module, x: torch.Tensor) -> LanguageBank:
    """The bank a forward of the batch `x` runs with; its refusals by name, before any device work."""
    bank = module.__dict__["_language_bank"]
    enc = module.encoder
    if module.training or enc.training or module.decoder.training:
        raise NotImplementedError("language bank: training with a language bank is not implemented (a train-mode forward); "
                                  "fine-tune one language on a module without a bank (adapter_finetuning) and language_bank_add() the result")
    if bank.precision != enc.precision:
        raise RuntimeError(f"language bank: the bank was created under precision={bank.precision!r} and holds operands of that mode; the encoder now "
                           f"runs precision={enc.precision!r}.  Set the precision before language_bank()")
    if x.shape[0] > LORA_BANK_MAX_CLIPS:
        raise RuntimeError(f"language bank: a batch of {x.shape[0]} clips; a forward with a language bank takes up to {LORA_BANK_MAX_CLIPS} (the bank's id buffer)")
    return bank


def decode(module, collapsed: torch.Tensor, counts: torch.Tensor) -> List[str]:
    """predict()'s strings: clip i decoded with the text transform of the language selected for it."""
    bank = module.__dict__["_language_bank"]
    slots = bank.slots(int(collapsed.shape[0]))
    if not any(slots):
        return bank.transforms[0].decode_collapsed(collapsed, counts)
    rows, n = collapsed.detach().to("cpu"), counts.detach().to("cpu")
    out: List[Optional[str]] = [None] * len(slots)
    for s in sorted(set(slots)):
        idx = [i for i, si in enumerate(slots) if si == s]
        for i, text in zip(idx, bank.transforms[s].decode_collapsed(rows[idx], n[idx])):
            out[i] = text
    return out
