"""BaseCTCModule -- the plugin surface of the reference's src/thunder/module.py:25-189.

Subclasses pytorch_lightning.LightningModule when Lightning is installed (it is not in this image), otherwise a
plain nn.Module with the same methods, so `pl.Trainer.fit` keeps working where available."""
from __future__ import annotations

import contextlib
from typing import Any, Dict, List, Optional, Tuple, Union

import torch
from torch import Tensor, nn

from . import _lib
from .ctc_loss import calculate_ctc
from .text_processing.transform import BatchTextTransformer

try:  # optional dependency of the reference
    import pytorch_lightning as pl
    _Base = pl.LightningModule
except Exception:  # pragma: no cover - Lightning is absent in the build image
    pl = None
    _Base = nn.Module


def greedy_decode(logits: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """argmax over classes + run-collapse on the GPU.  logits [B, V, T'] fp32 -> (ids [B, T'], collapsed [B, T'],
    counts [B]) int32."""
    if not logits.is_cuda:
        raise RuntimeError("greedy_decode: GPU tensors required (no CPU fallback)")
    b, v, t = logits.shape
    lg = logits
    if lg.dtype != torch.float32 or lg.stride(2) != 1 or lg.stride(0) != v * lg.stride(1):
        lg = lg.to(torch.float32).contiguous()
    ids = torch.empty(b, t, dtype=torch.int32, device=lg.device)
    # collapsed ids and their per-row counts share ONE buffer, so that the host takes them in a single device -> host copy
    # (BatchTextTransformer.decode_collapsed); the views behave like separate tensors for everyone else
    packed = torch.empty(b * t + b, dtype=torch.int32, device=lg.device)
    collapsed, counts = packed[: b * t].view(b, t), packed[b * t:]
    st = _lib.lib().ts_greedy_decode(lg.data_ptr(), b, v, t, lg.stride(1), ids.data_ptr(), collapsed.data_ptr(),
                                     counts.data_ptr(), torch.cuda.current_stream(lg.device).cuda_stream)
    _lib.check(st, "ts_greedy_decode")
    return ids, collapsed, counts


class BaseCTCModule(_Base):
    def __init__(self, encoder: nn.Module, decoder: nn.Module, audio_transform: nn.Module,
                 text_transform: BatchTextTransformer, optimizer_class=torch.optim.AdamW, optimizer_kwargs: Dict = None,
                 lr_scheduler_class=None, lr_scheduler_kwargs: Dict = None, encoder_final_dimension: int = None):
        super().__init__()
        self.encoder = encoder
        self.decoder = decoder
        self.audio_transform = audio_transform
        self.text_transform = text_transform
        self.optimizer_class = optimizer_class
        self.optimizer_kwargs = optimizer_kwargs or {}
        self.lr_scheduler_class = lr_scheduler_class
        self.lr_scheduler_kwargs = lr_scheduler_kwargs or {}
        self.lr_scheduler_interval = self.lr_scheduler_kwargs.pop("interval", "step")
        self.encoder_final_dimension = encoder_final_dimension
        try:  # under Lightning the metric objects must be torchmetrics.Metric instances (self.log takes them)
            if pl is None:
                raise ImportError
            from torchmetrics import CharErrorRate, WordErrorRate
        except Exception:  # otherwise: the same two error rates with the edit distances computed on the device
            from .metrics import CharErrorRate, WordErrorRate
        self.validation_cer, self.validation_wer = CharErrorRate(), WordErrorRate()
        self.example_input_array = (torch.randn((10, 16000)), torch.randint(100, 16000, (10,)))

    # ------------------------------------------------------------------------------------------------------------------
    # Inference as users call it (`module(x, lengths)` / `module.predict(x)` in eval mode under no_grad): the ~90 launches of a forward are
    # replayed from a hipGraph per input signature instead of being issued from Python one by one (no reference counterpart; the reference's
    # forward is module.py:74-86).  `graph_inference`: None = automatic (on for the model families whose whole forward is capture-safe: the
    # mel front end + QuartzNet / Citrinet encoder + this package's decoders), True / False = forced on / off.
    graph_inference: Optional[bool] = None
    # QuartzNet's last block (1x1 conv + BN + ReLU) and the conv1d decoder as one launch (thunder_speech_amd/qn_head.h) where the model has that
    # shape; False: the two launches of ts_tcs_subblock_fwd, always.  Part of the inference graphs' stamp.
    fused_head: bool = True
    MAX_INFERENCE_GRAPHS = 8             # graphs kept per module (outputs + at most one static input copy per signature; the launch arena is shared)

    def _inference_graph_ok(self, x: Tensor) -> bool:
        if not x.is_cuda or self.training or torch.is_grad_enabled() or self.graph_inference is False:
            return False
        if torch.cuda.is_current_stream_capturing():          # the caller is recording its own graph: launch into it
            return False
        if getattr(self, "_frozen_graph", None) is not None:  # graph_frozen_encoder() replays its own graph inside the forward
            return False
        auto = getattr(self, "_graph_auto", None)
        if auto is None:
            from .blocks import _Conv1dDecoder, _LinearDecoder
            from .quartznet.blocks import EncoderSequential
            from .quartznet.transform import _FilterbankFeatures as FilterbankFeatures
            auto = self._graph_auto = (isinstance(self.encoder, EncoderSequential) and isinstance(self.audio_transform, FilterbankFeatures)
                                       and isinstance(self.decoder, (_Conv1dDecoder, _LinearDecoder)))
        if not (self.graph_inference or auto):
            return False
        return not any(m.training for m in (self.encoder, self.decoder, self.audio_transform))

    def _weights_stamp(self):
        """Changes whenever a parameter / buffer of the model is written in place (optimizer step, load_state_dict, manual edits): the sum
        of the tensors' version counters.  The tensor list is rebuilt on train() / _apply() (.to, .half ...) / load_state_dict; code that
        REPLACES a Parameter object calls reset_inference_graphs().  An encoder that adds or removes Parameters of its own (LoRA:
        HuggingFaceEncoderAdapt.lora_finetuning / merge_lora) counts that in `_param_epoch`: the list is rebuilt when it moves, and it is part
        of the stamp."""
        ts = getattr(self, "_stamp_tensors", None)
        epoch = getattr(self.encoder, "_param_epoch", 0)
        if ts is None or self.__dict__.get("_stamp_epoch", 0) != epoch:
            ts = self._stamp_tensors = [t for m in (self.audio_transform, self.encoder, self.decoder)
                                        for t in list(m.parameters()) + list(m.buffers())]
            self.__dict__["_stamp_epoch"] = epoch
        return sum(t._version for t in ts) + (epoch << 48) + (int(bool(self.fused_head)) << 47)

    def reset_inference_graphs(self) -> None:
        self.__dict__.pop("_stamp_tensors", None)
        self.__dict__.pop("_infer_graphs", None)
        self.__dict__.pop("_graph_auto", None)
        self.__dict__.pop("_frozen_head", None)
        self.__dict__.pop("_auto_graphs", None)                    # predict_auto's table (huggingface/language_bank.py)

    def train(self, mode: bool = True):
        self.reset_inference_graphs()
        return super().train(mode)

    def _apply(self, fn, *args, **kwargs):
        self.reset_inference_graphs()
        return super()._apply(fn, *args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        self.reset_inference_graphs()
        return super().load_state_dict(*args, **kwargs)

    def _graphed_inference(self, x: Tensor, lengths: Tensor):
        """(logits, out_lengths, ids, collapsed, counts) -- the graph's OWN output buffers, overwritten by the next call of this signature --
        or None: this input has no graph (yet).  Two kinds of graph per input signature (shapes, dtypes, device):
          * zero-copy: reads the waveform where the caller's tensor lives (keyed by its address; captured the second time a signature is seen
            AT that address -- a serving loop whose batches land in the same allocation, or a few rotating buffers): no input copy per call;
          * copying: one per signature, the waveform is copied into the graph's static buffer first (61 MB at 64 x 15 s, ~1.5 % of a step);
            captured once a signature keeps arriving at new addresses.
        At most MAX_INFERENCE_GRAPHS graphs are kept; everything else runs eagerly (a shape that never repeats would pay three forward passes
        for nothing).  All captures of a module record on ONE side stream, so that re-captures (after a weight update) find the launch arena
        of the previous ones instead of growing a new one (tensors.arena is keyed by stream)."""
        from .utils import GraphedForward
        graphs = self.__dict__.get("_infer_graphs")
        stamp = self._weights_stamp()
        if graphs is None or graphs[0] != stamp:
            def run(xx, ll):
                logits, out_lengths = self._forward_eager(xx, ll)
                return (logits, out_lengths) + greedy_decode(logits)
            streams = self.__dict__.setdefault("_infer_streams", {})
            side = streams.get(str(x.device))
            if side is None:
                side = streams[str(x.device)] = torch.cuda.Stream(device=x.device)
            graphs = self.__dict__["_infer_graphs"] = (stamp, GraphedForward(run, stream=side, alias_first=True), GraphedForward(run, stream=side), {})
        _, gz, gc, seen = graphs
        if lengths.device != x.device:
            lengths = lengths.to(x.device)
        if not x.is_contiguous():
            x = x.contiguous()
        kz, kc = gz.signature(x, lengths), gc.signature(x, lengths)
        if gz.has(kz):
            return gz(x, lengths)
        room = gz.count() + gc.count() < self.MAX_INFERENCE_GRAPHS
        if len(seen) > 512:
            seen.clear()
        nz, nc = seen.get(kz, 0) + 1, seen.get(kc, 0) + 1
        seen[kz], seen[kc] = nz, nc
        if nz >= 2 and room:
            return gz(x, lengths)                         # second sighting of this shape at this address: zero-copy graph
        if gc.has(kc):
            return gc(x, lengths)
        if nc >= 4 and nz < 2 and room:
            return gc(x, lengths)                         # the shape keeps coming back at new addresses: one copying graph for it
        return None

    def forward(self, x: Tensor, lengths: Tensor) -> Tuple[Tensor, Optional[Tensor]]:
        """[batch, time] audio -> (logits [batch, vocab, time'] BEFORE softmax, output lengths)."""
        if self._inference_graph_ok(x):
            out = self._graphed_inference(x, lengths)
            if out is not None:
                return out[0].clone(), out[1].clone()      # the caller may keep them across calls: never hand out the graph's buffers
        return self._forward_eager(x, lengths)

    def _forward_eager(self, x: Tensor, lengths: Tensor) -> Tuple[Tensor, Optional[Tensor]]:
        if self.__dict__.get("_language_bank") is not None:
            return self._language_bank_forward(x, lengths)
        graphed = getattr(self, "_frozen_graph", None)
        if graphed is not None and x.is_cuda and not self.encoder.training and \
                not any(p.requires_grad for p in self.encoder.parameters()):
            if self._fused_head_ok(x):                             # inference on the frozen encoder: the same launches as without the graph
                return self._frozen_head_forward(x, lengths)
            encoded, out_lengths = graphed(x, lengths)             # front end + frozen encoder replayed from a hipGraph
            return self.decoder(encoded), out_lengths
        from . import tensors as _t
        with _t.lengths_scope():       # the front end's frame lengths reach the encoder with their int32 copy already made
            features, feature_lengths = self.audio_transform(x, lengths)
            if self._fused_head_ok(x):
                fused = self.encoder.forward_head(features, feature_lengths, self.decoder)
                if fused is not None:
                    return fused
            encoded, out_lengths = self.encoder(features, feature_lengths)
        return self.decoder(encoded), out_lengths

    def _language_bank_forward(self, x: Tensor, lengths: Tensor) -> Tuple[Tensor, Optional[Tensor]]:
        """The forward with a language bank (language_bank()): the encoder takes every clip's attention adapters from the bank, and
        ts_mms_lang_bank_head_fwd stands in place of the decoder -- logits [B, v_pad, T'], the classes beyond a clip's vocabulary at -1e30."""
        from . import tensors as _t
        from .huggingface import language_bank as LB
        bank = LB.check_forward(self, x)                           # the refusals, by name, before any device work
        with _t.lengths_scope():
            features, feature_lengths = self.audio_transform(x, lengths)
            encoded, out_lengths = self.encoder(features, feature_lengths)
        return bank.head(encoded.transpose(-1, -2)), out_lengths   # the encoder's [B, C, T'] is a view of its time-major result

    def _frozen_head_forward(self, x: Tensor, lengths: Tensor) -> Tuple[Tensor, Optional[Tensor]]:
        """graph_frozen_encoder() while the fused head applies: the graph ends in ts_qn_head_fwd instead of the last block, so a forward gives
        the bits it gives without the graph.  The decoder's packed weights are captured with it: the graph is dropped when they change (the
        decoder is what trains over a frozen encoder) and with the inference graphs (train(), .to(), load_state_dict)."""
        from .utils import GraphedForward
        dec = self.decoder
        key = tuple((t.data_ptr(), t._version) for t in (dec.weight, dec.bias))
        cur = self.__dict__.get("_frozen_head")
        if cur is None or cur[0] != key:
            cur = self.__dict__["_frozen_head"] = (key, GraphedForward(
                lambda xx, ll: self.encoder.forward_head(*self.audio_transform(xx, ll), dec)))
        logits, out_lengths = cur[1](x, lengths)
        return logits.clone(), out_lengths                         # the caller may keep them: never hand out the graph's buffer

    def _fused_head_ok(self, x: Tensor) -> bool:
        """The last encoder block and the decoder may run as one launch (EncoderSequential.forward_head): inference only (eval mode, no
        autograd, GPU), a QuartzNet-shaped end (EncoderSequential.head_block) in front of a conv1d decoder of at most 32 classes, and no
        forward hook that would want to see the tensor in between.  Whether the kernel takes the geometry is forward_head's business."""
        if not self.fused_head or not x.is_cuda or torch.is_grad_enabled():
            return False
        enc, dec = self.encoder, self.decoder
        if self.training or enc.training or dec.training:
            return False
        from .blocks import _Conv1dDecoder
        from .quartznet.blocks import EncoderSequential
        if not isinstance(enc, EncoderSequential) or type(dec) is not _Conv1dDecoder or dec.out_channels > 32:
            return False
        last = enc.head_block()
        if last is None or last.training or dec.in_channels != last.mconv[0].conv.out_channels:
            return False
        hooked = lambda m: bool(m._forward_hooks or m._forward_pre_hooks)
        return not (hooked(enc) or hooked(last) or hooked(dec))

    def graph_frozen_encoder(self, enable: bool = True) -> "BaseCTCModule":
        """Opt-in (no reference counterpart): while the encoder is frozen and in eval mode -- the first phase of the reference's
        fine-tuning recipe -- replay `audio_transform -> encoder` from a hipGraph (one per input shape) instead of launching its
        ~80 kernels from Python every step.  The encoder output then lives in the graph's buffer until the next forward."""
        from .utils import GraphedForward
        self._frozen_graph = GraphedForward(lambda x, lengths: self.encoder(*self.audio_transform(x, lengths))) if enable else None
        self.__dict__.pop("_frozen_head", None)
        return self

    def predict(self, x: Tensor) -> List[str]:
        """Greedy transcription; every clip is treated as full length (module.py:98)."""
        audio_lengths = torch.full((x.shape[0],), x.shape[-1], dtype=torch.int32, device=x.device)
        out = self._graphed_inference(x, audio_lengths) if self._inference_graph_ok(x) else None
        if out is not None:
            collapsed, counts = out[3], out[4]             # consumed right here: no copies
        else:
            pred, _ = self._forward_eager(x, audio_lengths)
            _, collapsed, counts = greedy_decode(pred)
        if self.__dict__.get("_language_bank") is not None:
            from .huggingface import language_bank as LB
            return LB.decode(self, collapsed, counts)              # clip i with the text transform of the language selected for it
        return self.text_transform.decode_collapsed(collapsed, counts)

    def predict_adapted(self, x: Tensor, adapters) -> List[str]:
        """predict(x) with clip i served by the LoRA adaptation `adapters[i]` of the encoder's bank (a name, or None for the base alone;
        HuggingFaceEncoderAdapt.lora_bank / lora_bank_add); the selection that held before the call holds again after it.  No reference
        counterpart.  predict, forward, align, predict_spans, predict_beam and predict_nbest see whatever selection is current."""
        if not hasattr(self.encoder, "select_adapters"):
            raise NotImplementedError(f"predict_adapted: the encoder ({type(self.encoder).__name__}) serves no LoRA bank (HuggingFaceEncoderAdapt does)")
        previous = self.encoder.selected_adapters()
        self.encoder.select_adapters(adapters)
        try:
            return self.predict(x)
        finally:
            self.encoder.select_adapters(previous)

    # ------------------------------------------------------------------------------------------------------------------
    # Many MMS languages on one module (no reference counterpart; huggingface/language_bank.py, csrc/mms_lang_bank.hip): a bank of language packs
    # -- the attention adapters of every layer and a CTC head -- next to the one packed base of an MMS checkpoint; every clip of a batch picks
    # its language by name.  The bank's tensors are plain attributes at fixed addresses (state_dict() does not change): adding, removing and
    # selecting write in place, so captured graphs keep replaying.  A module without a bank runs the launches it ran before.
    def language_bank(self, name: str, capacity: int = 8, max_vocab: Optional[int] = None) -> None:
        """Create a bank of `capacity` language slots and put the language this module was loaded with -- the encoder's attention adapters,
        `decoder[2]` and `text_transform` as they are now -- into slot 0 under `name`: the resident language, which serves every clip that
        selects nothing else and cannot be removed.  `max_vocab`: the largest vocabulary the bank takes (a multiple of 16; default: the
        resident vocabulary rounded up); forward() then returns [B, max_vocab, T'] with the classes beyond a clip's vocabulary at -1e30.
        Refused by name: an encoder without attention adapters, precision="mxfp8", a second bank."""
        from .huggingface import language_bank as LB
        LB.create(self, name, capacity, max_vocab)

    def language_bank_add(self, lang: str, adapter_sd: Dict[str, Tensor], tokens: List[str]) -> int:
        """Put a language into a free slot: `adapter_sd` with exactly the keys of transformers' `model._get_adapters()` (the contents of an
        adapter.<lang>.safetensors: the attention adapters and lm_head), `tokens` its vocabulary in id order.  Returns the slot.  Written in
        place: captured graphs stay valid.  Refused by name: a duplicate name, a full bank, wrong keys or shapes, a vocabulary larger than
        max_vocab, a blank index other than the resident language's (the greedy decode of a batch has one blank)."""
        from .huggingface import language_bank as LB
        return LB.add(self, lang, adapter_sd, tokens)

    def language_bank_load(self, model_dir: str, langs) -> List[int]:
        """language_bank_add for each of `langs` from a local checkpoint directory: adapter.{lang}.safetensors and that language's entry of the
        nested vocab.json.  Returns the slots."""
        from .huggingface import language_bank as LB
        return LB.load(self, model_dir, langs)

    def language_bank_remove(self, lang: str) -> None:
        """Zero and free the slot of `lang`; clips that selected it go back to the resident language.  Slot 0 cannot be removed."""
        from .huggingface import language_bank as LB
        LB.remove(self, lang)

    def language_bank_names(self) -> List[str]:
        """The languages in the bank, in slot order (the resident one first)."""
        from .huggingface import language_bank as LB
        return LB.names(self)

    def select_languages(self, langs) -> None:
        """One entry per clip of the batches to come: a language of the bank, or None for the resident one; clips beyond the given entries get
        the resident language.  One host-to-device copy into the bank's id buffer: nothing is re-captured."""
        from .huggingface import language_bank as LB
        LB.select(self, langs)

    def selected_languages(self) -> List[Optional[str]]:
        """What select_languages() was last given (a copy; [] after language_bank())."""
        from .huggingface import language_bank as LB
        return list(LB._bank(self, "selected_languages").selection)

    def predict_languages(self, x: Tensor, langs) -> List[str]:
        """predict(x) with clip i served by the language `langs[i]` of the bank (None: the resident one) and decoded with that language's
        vocabulary; the selection that held before the call holds again after it."""
        previous = self.selected_languages()
        self.select_languages(langs)
        try:
            return self.predict(x)
        finally:
            self.select_languages(previous)

    def language_router(self, classifier, mapping: Optional[Dict[str, str]] = None) -> None:
        """Attach an AudioClassifierModule (huggingface/classification.py: an MMS language-identification checkpoint) that picks every clip's
        language on the device.  `mapping`: {classifier label: bank language}, default the identity.  Classes of languages the bank does not
        hold route to the resident language; language_bank_add / language_bank_remove rewrite the routing table in place, so a captured graph
        routes to a language added after its capture.  Refused by name: no bank, a mapping that names a label the classifier does not have,
        differing sample rates."""
        from .huggingface import language_bank as LB
        LB.attach_router(self, classifier, mapping)

    def identify_languages(self, x: Tensor) -> List[Optional[str]]:
        """The routed language of every clip: the bank language of the classifier's most probable class among the classes mapped to a language
        in the bank; None when there is no such class (the resident language serves the clip)."""
        from .huggingface import language_bank as LB
        return LB.identify(self, x)

    def predict_auto(self, x: Tensor) -> Tuple[List[str], List[str]]:
        """(texts, languages): predict(x) with every clip served by the language the attached classifier routes it to, and that language.  One
        captured graph per input signature holds the classifier and the ASR forward; the classifier's head writes the slots into the bank's id
        buffer on the device, so no host work happens between the two encoders.  The selection that held before the call holds again after."""
        from .huggingface import language_bank as LB
        return LB.predict_auto(self, x)

    def _one_language(self, what: str) -> None:
        """`what` turns text into ids, or carries an LM, of one language: refused by name while any clip selects a non-resident language."""
        if self.__dict__.get("_language_bank") is not None:
            from .huggingface import language_bank as LB
            LB.refuse_mixed(self, what)

    # ------------------------------------------------------------------------------------------------------------------
    # "When was it said" (no reference counterpart): forced alignment of known transcripts and the spans of the greedy transcript, on the
    # kernels of csrc/ctc_align.hip (ctc_align.py).  predict() / forward() above are untouched.
    @property
    def sample_rate(self) -> int:
        """Samples per second of the waveforms the module takes (host only): the front end's `sample_rate` where it records one, else 16 000
        (every checkpoint family this package loads)."""
        return int(getattr(self.audio_transform, "sample_rate", 16000))

    @property
    def samples_per_frame(self) -> int:
        """Waveform samples per frame of the logits (host only): frame f starts at f * samples_per_frame / sample_rate seconds.  Mel front
        end: n_window_stride x the encoder's total stride; transformers families: prod(conv_stride) (SEW's squeeze and upsampler cancel),
        times adapter_stride ** num_adapter_layers with add_adapter."""
        cfg = getattr(getattr(self.encoder, "original_encoder", None), "config", None)
        if cfg is not None:
            n = 1
            for s in cfg.conv_stride:
                n *= int(s)
            if getattr(cfg, "add_adapter", False):
                n *= int(cfg.adapter_stride) ** int(cfg.num_adapter_layers)
            return n
        from .quartznet.blocks import MaskedConv1d
        hops = [m.hop_length for m in self.audio_transform.modules() if hasattr(m, "hop_length")]
        if len(hops) != 1:
            raise NotImplementedError("samples_per_frame: the audio transform is neither the mel front end nor a transformers one")
        n = int(hops[0])
        for blk in self.encoder.children():
            main = getattr(blk, "mconv", blk)                     # the main path of a block (its residual branch has strides of its own)
            for m in main.modules():
                if isinstance(m, MaskedConv1d):
                    n *= int(m.stride)
        return n

    @contextlib.contextmanager
    def _eval_no_grad(self):
        """Eval mode and no_grad for the forwards inside; afterwards every submodule gets its own flag back (a frozen encoder stays in eval mode)."""
        modes = [(m, m.training) for m in self.modules()]
        if any(on for _, on in modes):
            self.eval()
        try:
            with torch.no_grad():
                yield
        finally:
            if any(on for _, on in modes):
                for m, on in modes:
                    m.training = on
                self.reset_inference_graphs()

    def _eval_logits(self, x: Tensor, lengths: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
        """(logits, output lengths) of the eval-mode forward under no_grad; lengths None: every clip is full length, as predict()."""
        if not x.is_cuda:
            raise RuntimeError("align / predict_spans: GPU tensors required (no CPU fallback)")
        if lengths is None:
            lengths = torch.full((x.shape[0],), x.shape[-1], dtype=torch.int32, device=x.device)
        with self._eval_no_grad():
            logits, out_lengths = self(x, lengths)
        if out_lengths is None:
            out_lengths = torch.full((x.shape[0],), logits.shape[-1], dtype=torch.int32, device=x.device)
        return logits, out_lengths

    def align(self, x: Tensor, texts: List[str], lengths: Optional[Tensor] = None) -> List["AlignedClip"]:
        """Forced alignment of `texts` to the clips `x` [batch, time]: per clip the score (sum of the best path's log-probabilities) and
        one TokenSpan per token of the encoded transcript (token, start / end in seconds and in frames, log-probability).  A transcript that
        does not fit its clip gives score -inf and no tokens instead of raising: one bad transcript does not fail a batch."""
        self._one_language("align")
        from . import ctc_align as A
        logits, out_lengths = self._eval_logits(x, lengths)
        y, y_lengths = self.text_transform.encode(list(texts), device=x.device)
        al = A.forced_align(logits, y, out_lengths, y_lengths, self.text_transform.vocab.blank_idx)
        ids, spans, logp, counts, scores = A._to_host(al.targets, al.spans, al.span_logp, al.target_lengths, al.score)     # one copy
        counts = [0 if scores[b] == float("-inf") else int(counts[b]) for b in range(len(counts))]
        return A.clips_from_spans(ids, spans, logp, counts, scores, self.text_transform.vocab.itos, self.samples_per_frame, self.sample_rate)

    def predict_spans(self, x: Tensor) -> List["AlignedClip"]:
        """predict() with the positions kept: per clip the tokens of the greedy transcript (blank runs dropped) with their spans; joining
        the tokens, with the separators read as spaces, gives predict(x) as called under no_grad (this method always runs the inference
        forward; predict() follows the caller's grad mode, and a decoder with trainable parameters takes its f32 training path under grad).
        The clip's score is the sum of its tokens' log-probabilities."""
        self._one_language("predict_spans")
        from . import ctc_align as A
        logits, _ = self._eval_logits(x, None)
        gs = A.greedy_spans(logits, None, self.text_transform.vocab.blank_idx)
        ids, spans, logp, counts = A._to_host(gs.tokens, gs.spans, gs.span_logp, gs.counts)                              # one copy
        scores = [float(logp[b, : int(counts[b])].sum()) for b in range(len(counts))]
        return A.clips_from_spans(ids, spans, logp, counts, scores, self.text_transform.vocab.itos, self.samples_per_frame, self.sample_rate)

    # ------------------------------------------------------------------------------------------------------------------
    # CTC prefix beam search (no reference counterpart), on the kernels of csrc/ctc_beam.hip (ctc_beam.py).  predict() is untouched.
    def _beam_search_on(self, what: str, logits: Tensor, lengths: Optional[Tensor], n_best: int, beam_width: int, token_cap: int, lm, alpha: float,
                        beta: float, oov_score: float, hotword_weight: float, boosts):
        """The search that `lm`'s type asks for, on `logits` with their `lengths` (None: every frame): none, the token-level ctc_lm.NGramLM, the
        word-level ctc_lm.WordNGramLM with its lexicon and hot words, or -- for a sentencepiece vocabulary -- ctc_lm.PieceWordNGramLM.  `logits`
        may be a function that returns (logits, lengths): the keywords are checked before it runs."""
        self._one_language(what)
        from . import ctc_beam as B
        from . import ctc_lm as M
        vocab = self.text_transform.vocab
        blank, word_level, piece_level = vocab.blank_idx, isinstance(lm, M.WordNGramLM), isinstance(lm, M.PieceWordNGramLM)
        if word_level:
            shown = [c for c, tok in enumerate(vocab.itos) if tok == " " and c != blank]
            if not shown or shown[0] != lm.delimiter:
                raise ValueError(f"{what}: the LM ends a word at class {lm.delimiter}, this module's vocabulary shows " +
                                 (f"class {shown[0]}" if shown else "no class") + " as ' '")
        elif piece_level:
            if lm.blank_idx != blank:
                raise ValueError(f"{what}: the LM was compiled with the blank at class {lm.blank_idx}, this module's blank is class {blank}")
            differs = [c for c, (mine, its) in enumerate(zip(vocab.itos, lm.itos)) if mine != its]
            if differs or len(lm.itos) != len(vocab.itos):
                c = differs[0] if differs else min(len(lm.itos), len(vocab.itos))
                show = lambda itos: repr(itos[c]) if c < len(itos) else "no such class"
                raise ValueError(f"{what}: the LM was compiled for another vocabulary: class {c} is {show(lm.itos)} there and {show(vocab.itos)} "
                                 "in this module")
        elif (oov_score, hotword_weight, boosts) != (-10.0, 0.0, None):
            raise ValueError(f"{what}: oov_score, hotword_weight and boosts belong to a ctc_lm.WordNGramLM or a ctc_lm.PieceWordNGramLM; this "
                             "search has no lexicon")
        if callable(logits):
            logits, lengths = logits()
        if word_level:
            return M.beam_search_word_lm(logits, lm, alpha, beta, lengths, blank, beam_width, token_cap, n_best, True, oov_score, hotword_weight, boosts)
        if piece_level:
            return M.beam_search_piece_lm(logits, lm, alpha, beta, lengths, blank, beam_width, token_cap, n_best, True, oov_score, hotword_weight, boosts)
        if lm is None:
            return B.beam_search(logits, lengths, blank, beam_width, token_cap, n_best)
        return M.beam_search_lm(logits, lm, alpha, beta, lengths, blank, beam_width, token_cap, n_best)

    def _beam_search(self, what: str, x: Tensor, n_best: int, beam_width: int, token_cap: int, lm, alpha: float, beta: float, oov_score: float,
                     hotword_weight: float, boosts):
        """_beam_search_on the clips `x`, every clip full length."""
        return self._beam_search_on(what, lambda: (self._eval_logits(x, None)[0], None), None, n_best, beam_width, token_cap, lm, alpha, beta,
                                    oov_score, hotword_weight, boosts)

    def predict_beam(self, x: Tensor, beam_width: int = 16, token_cap: int = 8, lm=None, alpha: float = 0.5, beta: float = 1.0,
                     oov_score: float = -10.0, hotword_weight: float = 0.0, boosts=None) -> List[str]:
        """Transcription by CTC prefix beam search: per clip the transcript whose alignments carry the most probability among the
        `beam_width` prefixes kept per frame (predict() follows the single best path instead).  Every clip is treated as full length.
        With `lm` (a ctc_lm.NGramLM over this module's classes) the n-gram LM is fused into the search on the kernels of
        csrc/ctc_beam_lm.hip: LM weight `alpha`, token bonus `beta`.  With a ctc_lm.WordNGramLM (a word-level LM over a character
        vocabulary) the search is that of csrc/ctc_beam_word_lm.hip: `beta` is a word bonus, `oov_score` what a word outside the lexicon
        pays, `hotword_weight` the boost of every hot word and `boosts` a hot word's own.  A ctc_lm.PieceWordNGramLM does the same for a
        sentencepiece vocabulary on csrc/ctc_beam_piece_lm.hip (a word ends where a piece that starts the next one follows); only these
        two LMs take the three keywords."""
        from . import ctc_align as A
        res = self._beam_search("predict_beam", x, 1, beam_width, token_cap, lm, alpha, beta, oov_score, hotword_weight, boosts)
        ids, counts = A._to_host(res.tokens[:, 0], res.lengths[:, 0])                                                    # one copy
        return self.text_transform.decode_collapsed(torch.from_numpy(ids), torch.from_numpy(counts))

    def predict_nbest(self, x: Tensor, n_best: int, beam_width: int = 16, token_cap: int = 8, lm=None, alpha: float = 0.5,
                      beta: float = 1.0, oov_score: float = -10.0, hotword_weight: float = 0.0, boosts=None) -> List[List["Hypothesis"]]:
        """The `n_best` best transcripts of each clip under CTC prefix beam search, best first: text, score (log of the summed probability
        of the transcript's surviving alignments) and per token the frame and time at which it entered the hypothesis.  With `lm` the
        search is the fused one of predict_beam: `score` is the fused score and every hypothesis carries `lm_score`, the unweighted
        log10 LM score of its tokens (its words, for a WordNGramLM) and </s>.  A PieceWordNGramLM gives hypotheses of pieces: two
        segmentations of one text are two hypotheses."""
        from . import ctc_align as A
        from . import ctc_beam as B
        res = self._beam_search("predict_nbest", x, n_best, beam_width, token_cap, lm, alpha, beta, oov_score, hotword_weight, boosts)
        if lm is None:
            tokens, frames, lengths, scores, counts = A._to_host(res.tokens, res.frames, res.lengths, res.scores, res.counts)  # one copy
            lm_scores = None
        else:
            tokens, frames, lengths, scores, counts, lm_scores = A._to_host(res.tokens, res.frames, res.lengths, res.scores, res.counts,
                                                                            res.lm_scores)                                # one copy
        return B.hypotheses_from_tables(tokens, frames, lengths, scores, counts, self.text_transform.vocab.itos, self.text_transform._ids_to_text,
                                        self.samples_per_frame, self.sample_rate, lm_scores)

    # ------------------------------------------------------------------------------------------------------------------
    # Recordings longer than one forward pass (no reference counterpart: module.py:88-100 takes one batch): overlapping full-length windows
    # on the captured inference graph of ONE signature, stitched back onto the recording's frame grid (longform.py, csrc/longform.hip), and
    # the existing decoders, plus the long aligner (csrc/ctc_align_long.hip), on the stitched logits.  The methods above are untouched.
    def _frames_of(self, n_samples: int) -> int:
        """Output frames of a clip of `n_samples` samples by the module's own length arithmetic (host only: the front end's and the encoder's
        length functions on a CPU tensor)."""
        lengths = torch.tensor([int(n_samples)])
        cfg = getattr(getattr(self.encoder, "original_encoder", None), "config", None)
        if cfg is not None:
            from .huggingface.encoder import feat_extract_output_lengths
            adapters = int(cfg.num_adapter_layers) if getattr(cfg, "add_adapter", False) else 0
            return int(feat_extract_output_lengths(cfg.conv_kernel, cfg.conv_stride, lengths, adapters, int(getattr(cfg, "adapter_stride", 2))))
        front = [m for m in self.audio_transform.modules() if hasattr(m, "get_sequence_length")]
        if len(front) != 1:
            raise NotImplementedError("logits_long: the audio transform is neither the mel front end nor a transformers one")
        lengths = front[0].get_sequence_length(lengths)
        for blk in self.encoder.children():
            main = getattr(blk, "mconv", blk)
            for m in main.modules():
                if hasattr(m, "get_seq_len") and hasattr(m, "stride"):
                    lengths = m.get_seq_len(lengths)
        return int(lengths)

    def _long_recordings(self, what: str, recordings) -> List[Tensor]:
        recs = [recordings] if isinstance(recordings, Tensor) else list(recordings)
        if not recs:
            raise ValueError(f"{what}: no recordings")
        for r in recs:
            if not isinstance(r, Tensor) or r.dim() != 1 or r.numel() == 0:
                raise ValueError(f"{what}: every recording is a 1-D waveform tensor with at least one sample")
            if not r.is_cuda:
                raise RuntimeError(f"{what}: GPU tensors required (no CPU fallback)")
            if r.dtype != torch.float32:
                raise ValueError(f"{what}: float32 waveforms required")
        return recs

    def logits_long(self, recordings, chunk_s: float = 20.0, context_s: float = 2.0, batch_size: int = 16) -> "LongLogits":
        """The logits of recordings of any length on each recording's own frame grid: LongLogits(logits f32 [R, V, T_max], lengths int32 [R],
        plans).  `recordings`: a 1-D GPU f32 waveform or a list of them.  A recording longer than `chunk_s` seconds is run as overlapping
        windows of that length, `context_s` seconds of every window's ends discarded in favour of its neighbour (longform.plan_windows); the
        windows of all recordings are pooled and run `batch_size` at a time through the eval-mode forward under no_grad, entering through one
        staging buffer, so the inference graph of that one signature is captured once and replayed; one launch stitches the windows' logits.
        Nothing synchronises with the host between the batches.  A recording that fits one window runs as one clip of its own length: its row
        is what `module(x[None], ...)` gives.  A LoRA bank selection (select_adapters) holds for every batch of windows as it does for predict:
        entry i serves row i of each batch."""
        self._one_language("logits_long (transcribe_long, predict_spans_long, align_long)")
        from . import longform as LF
        recs = self._long_recordings("logits_long", recordings)
        dev, spf, sr = recs[0].device, self.samples_per_frame, self.sample_rate
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError("logits_long: batch_size must be at least 1")
        chunk = int(round(float(chunk_s) * sr))
        context = int(round(float(context_s) * sr / spf))
        if chunk < spf:
            raise ValueError(f"logits_long: chunk_s = {chunk_s} is shorter than one frame ({spf} samples)")
        frames = self._frames_of(chunk)
        multiple = LF.grid_multiple(getattr(getattr(self.encoder, "original_encoder", None), "config", None))
        plans = [LF.plan_windows(int(r.shape[0]), chunk, context, spf, frames, multiple) for r in recs]      # refusals before any device work
        table = [(i, s) for i, p in enumerate(plans) if p is not None for s in p.starts]
        short = [i for i, p in enumerate(plans) if p is None]
        with self._eval_no_grad():
            short_out = []
            for i in short:
                x = recs[i][None]
                lg, ln = self(x, torch.full((1,), x.shape[-1], dtype=torch.int32, device=dev))
                short_out.append((i, lg, ln))
            win = None
            if table:
                audio, rec_begin, _ = LF.pack_recordings(recs)
                n_win = len(table)
                n_batches = -(-n_win // batch_size)
                windows = torch.tensor(table + [(0, 0)] * (n_batches * batch_size - n_win), dtype=torch.int64).to(dev, non_blocking=True)
                stages = self.__dict__.setdefault("_long_stages", {})
                stage = stages.get((batch_size, chunk, str(dev)))
                if stage is None:                                  # kept: the zero-copy graph is keyed by this address
                    stages.clear()
                    stage = stages[(batch_size, chunk, str(dev))] = torch.zeros(batch_size, chunk, dtype=torch.float32, device=dev)
                full = torch.full((batch_size,), chunk, dtype=torch.int32, device=dev)
                for k in range(n_batches):
                    rows = min(batch_size, n_win - k * batch_size)
                    LF.gather_windows(audio, rec_begin, windows[k * batch_size:], rows, stage)
                    lg, _ = self(stage, full)
                    if win is None:
                        if lg.shape[-1] != frames:
                            raise RuntimeError(f"logits_long: the forward returned {lg.shape[-1]} frames for a window of {chunk} samples, the "
                                               f"module's length arithmetic says {frames}")
                        win = torch.empty(n_batches * batch_size, lg.shape[1], frames, dtype=lg.dtype, device=dev)
                    win[k * batch_size: (k + 1) * batch_size].copy_(lg)
        n_classes = win.shape[1] if win is not None else short_out[0][1].shape[1]
        t_max = max([p.n_frames for p in plans if p is not None] + [lg.shape[-1] for _, lg, _ in short_out])
        logits = torch.zeros(len(recs), n_classes, t_max, dtype=torch.float32, device=dev)
        lengths = torch.zeros(len(recs), dtype=torch.int32, device=dev)
        for i, lg, ln in short_out:
            logits[i, :, : lg.shape[-1]].copy_(lg[0])
            lengths[i: i + 1].copy_(ln if ln is not None else torch.full((1,), lg.shape[-1], dtype=torch.int32, device=dev))
        if win is not None:
            cuts = torch.tensor(LF.cut_table(plans), dtype=torch.int32).to(dev, non_blocking=True)
            LF.stitch_windows(win[: len(table)], cuts, logits, lengths)
        return LF.LongLogits(logits, lengths, plans)

    def transcribe_long(self, recordings, chunk_s: float = 20.0, context_s: float = 2.0, batch_size: int = 16, beam_width: Optional[int] = None,
                        token_cap: int = 8, lm=None, alpha: float = 0.5, beta: float = 1.0, oov_score: float = -10.0, hotword_weight: float = 0.0,
                        boosts=None) -> List[str]:
        """One transcript per recording of any length (logits_long).  beam_width None: greedy (the spans of ctc_align.greedy_spans on the
        stitched logits and their lengths, joined); otherwise the prefix beam search that `lm`'s type asks for, with predict_beam's keywords.  A
        ctc_lm.PieceWordNGramLM is taken as there."""
        from . import ctc_align as A
        if beam_width is None:
            if lm is not None or (oov_score, hotword_weight, boosts) != (-10.0, 0.0, None):
                raise ValueError("transcribe_long: lm, oov_score, hotword_weight and boosts belong to the beam search; give a beam_width")
            ll = self.logits_long(recordings, chunk_s, context_s, batch_size)
            gs = A.greedy_spans(ll.logits, ll.lengths, self.text_transform.vocab.blank_idx)
            return self.text_transform.decode_collapsed(gs.tokens, gs.counts)

        def stitched():
            ll = self.logits_long(recordings, chunk_s, context_s, batch_size)
            return ll.logits, ll.lengths
        res = self._beam_search_on("transcribe_long", stitched, None, 1, beam_width, token_cap, lm, alpha, beta, oov_score, hotword_weight, boosts)
        ids, counts = A._to_host(res.tokens[:, 0], res.lengths[:, 0])                                                    # one copy
        return self.text_transform.decode_collapsed(torch.from_numpy(ids), torch.from_numpy(counts))

    def predict_spans_long(self, recordings, chunk_s: float = 20.0, context_s: float = 2.0, batch_size: int = 16) -> List["AlignedClip"]:
        """predict_spans for recordings of any length: the tokens of the greedy transcript with their spans; times are absolute in the
        recording (the stitched grid is the recording's)."""
        from . import ctc_align as A
        ll = self.logits_long(recordings, chunk_s, context_s, batch_size)
        gs = A.greedy_spans(ll.logits, ll.lengths, self.text_transform.vocab.blank_idx)
        ids, spans, logp, counts = A._to_host(gs.tokens, gs.spans, gs.span_logp, gs.counts)                              # one copy
        scores = [float(logp[b, : int(counts[b])].sum()) for b in range(len(counts))]
        return A.clips_from_spans(ids, spans, logp, counts, scores, self.text_transform.vocab.itos, self.samples_per_frame, self.sample_rate)

    def align_long(self, recordings, texts: List[str], chunk_s: float = 20.0, context_s: float = 2.0, batch_size: int = 16) -> List["AlignedClip"]:
        """align for recordings of any length and transcripts of up to 32 767 tokens (ctc_align.forced_align_long on the stitched logits):
        per recording the score and one TokenSpan per token, times absolute in the recording.  A transcript that does not fit its recording
        gives score -inf and no tokens."""
        from . import ctc_align as A
        texts = list(texts)
        ll = self.logits_long(recordings, chunk_s, context_s, batch_size)
        if len(texts) != ll.logits.shape[0]:
            raise ValueError(f"align_long: {len(texts)} texts for {ll.logits.shape[0]} recordings")
        y, y_lengths = self.text_transform.encode(texts, device=ll.logits.device)
        al = A.forced_align_long(ll.logits, y, ll.lengths, y_lengths, self.text_transform.vocab.blank_idx)
        ids, spans, logp, counts, scores = A._to_host(al.targets, al.spans, al.span_logp, al.target_lengths, al.score)     # one copy
        counts = [0 if scores[b] == float("-inf") else int(counts[b]) for b in range(len(counts))]
        return A.clips_from_spans(ids, spans, logp, counts, scores, self.text_transform.vocab.itos, self.samples_per_frame, self.sample_rate)

    def training_step(self, batch, batch_idx: int) -> torch.Tensor:
        audio, audio_lengths, texts = batch
        y, y_lengths = self.text_transform.encode(texts, device=audio.device)
        probabilities, prob_lengths = self(audio, audio_lengths)
        loss = calculate_ctc(probabilities, y, prob_lengths, y_lengths, self.text_transform.vocab.blank_idx)
        if pl is not None:
            self.log("loss/train_loss", loss)
        return loss

    def validation_step(self, batch, batch_idx: int) -> torch.Tensor:
        audio, audio_lengths, texts = batch
        y, y_lengths = self.text_transform.encode(texts, device=audio.device)
        probabilities, prob_lengths = self(audio, audio_lengths)
        loss = calculate_ctc(probabilities, y, prob_lengths, y_lengths, self.text_transform.vocab.blank_idx)
        _, collapsed, counts = greedy_decode(probabilities)
        decoded_preds = self.text_transform.decode_collapsed(collapsed, counts)
        decoded_targets = self.text_transform.decode_prediction(y, remove_repeated=False)
        self.validation_cer(decoded_preds, decoded_targets)
        self.validation_wer(decoded_preds, decoded_targets)
        if pl is not None:
            self.log("loss/val_loss", loss)
            self.log("metrics/cer", self.validation_cer, on_epoch=True)
            self.log("metrics/wer", self.validation_wer, on_epoch=True)
        return loss

    def _resolve_builder_kwargs(self, kwargs: Dict) -> Dict:
        """The reference's one magic key (module.py:165-171): {"total_steps_arg": name} means "pass the trainer's estimated number of
        optimizer steps under `name`" (e.g. OneCycleLR's total_steps).  Everything else goes to the builder untouched."""
        name = kwargs.get("total_steps_arg")
        resolved = {k: v for k, v in kwargs.items() if k != "total_steps_arg"}
        if name:
            resolved[name] = self.trainer.estimated_stepping_batches
        return resolved

    def _update_special_optimizer_arg(self, kwargs: Dict) -> Dict:
        """The reference's hook name (module.py:165-171) and the one `configure_optimizers` calls: a subclass that overrides it is honoured."""
        return self._resolve_builder_kwargs(kwargs)

    def configure_optimizers(self) -> Union[torch.optim.Optimizer, Dict[str, Any]]:
        """Lightning contract (module.py:173-189): the optimizer over the trainable parameters, alone or with its scheduler entry."""
        trainable = [p for p in self.parameters() if p.requires_grad]
        optimizer = self.optimizer_class(trainable, **self._update_special_optimizer_arg(self.optimizer_kwargs))
        if self.lr_scheduler_class is None:
            return optimizer
        scheduler = self.lr_scheduler_class(optimizer, **self._update_special_optimizer_arg(self.lr_scheduler_kwargs))
        return dict(optimizer=optimizer, lr_scheduler=dict(scheduler=scheduler, interval=self.lr_scheduler_interval))
