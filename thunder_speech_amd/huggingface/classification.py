"""HuggingFace audio classification checkpoints -> AudioClassifierModule (no reference counterpart: the reference loads AutoModelForCTC only;
include_open/thunder_speech_amd/seq_cls.h, csrc/seq_cls.hip).

transformers' `...ForSequenceClassification` over wav2vec2, hubert, wavlm, data2vec-audio, unispeech(-sat), sew and the rotary wav2vec2-conformer
-- the MMS language-identification checkpoints (facebook/mms-lid-126 ... -4017), the SUPERB keyword / intent / emotion checkpoints -- is the
encoder, a mean over the valid frames, a projector and a classifier.  transformers keeps owning the weights, so the state-dict keys are its
own; the arithmetic runs on the HIP path: `HuggingFaceEncoderAdapt`'s plan for the encoder, ts_seq_cls_pool for the mean and ts_seq_cls_head
for projector, classifier, arg-max and its log-softmax.  Pool, layer sum and projector are linear, so the pool runs first and
`config.use_weighted_layer_sum` is one pool launch per hidden state, accumulating with the soft-maxed layer weight read on the device: no
[B][T][C] layer sum is formed.  Nothing here falls back to the transformers forward pass.

Out of scope: fine-tuning classification heads (train mode is refused: the head has no backward here); the ...ForAudioFrameClassification and
...ForXVector heads; sew-d and relative-position conformers (refused as before); a confidence threshold or fallback policy for the router
(huggingface/language_bank.py); LM fusion, alignment and long-form transcription under a routed selection; downloading checkpoints."""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Tuple

import torch
from torch import nn

from .. import _lib, tensors as _t
from .encoder import HuggingFaceEncoderAdapt, feat_extract_output_lengths
from .transform import Wav2Vec2Preprocess

__all__ = ["AudioClassifierModule", "classifier_from_huggingface", "load_huggingface_classifier"]

# ts_seq_cls_pool / ts_seq_cls_head: hidden size a multiple of 8 up to 4096, projector size a multiple of 16 up to 4096, up to 8192 labels
MAX_HIDDEN, MAX_PROJ, MAX_LABELS = 4096, 4096, 8192
# the plans with a tap for transformers' hidden_states (Wav2Vec2Plan.forward): everything but the conformer and SEW plans
NO_TAP_MODEL_TYPES = ("wav2vec2-conformer", "sew")


def _check_head(cfg, hidden: int, p: int, n_labels: int) -> None:
    """The head's refusals, by name; no device work."""
    bad = []
    if hidden % 8 or hidden > MAX_HIDDEN:
        bad.append(f"hidden_size={hidden} (the pooling kernel takes a multiple of 8 up to {MAX_HIDDEN})")
    if p % 16 or p > MAX_PROJ:
        bad.append(f"classifier_proj_size={p} (the head kernel takes a multiple of 16 up to {MAX_PROJ})")
    if n_labels < 1 or n_labels > MAX_LABELS:
        bad.append(f"num_labels={n_labels} (the head kernel takes 1 to {MAX_LABELS} classes)")
    if getattr(cfg, "use_weighted_layer_sum", False) and getattr(cfg, "model_type", "wav2vec2") in NO_TAP_MODEL_TYPES:
        bad.append(f"use_weighted_layer_sum=True with model_type={cfg.model_type!r} (the conformer and SEW plans do not expose their hidden states; "
                   "last-hidden-state pooling runs on them)")
    if bad:
        raise NotImplementedError("audio classification HIP path: unsupported configuration: " + ", ".join(bad))


class AudioClassifierModule(nn.Module):
    """encoder: a HuggingFaceEncoderAdapt around `model.base_model`; audio_transform: Wav2Vec2Preprocess; projector, classifier (nn.Linear) and
    layer_weights (a Parameter, or None without config.use_weighted_layer_sum): transformers' own, under its state-dict keys; labels:
    config.id2label in id order.  forward / predict / predict_topk run in eval mode only."""

    graph_inference: bool = True         # predict / predict_topk replay one hipGraph per input signature (False: launch from Python every call)

    def __init__(self, encoder: HuggingFaceEncoderAdapt, audio_transform: nn.Module, projector: nn.Linear, classifier: nn.Linear,
                 labels: List[str], layer_weights: Optional[nn.Parameter] = None):
        super().__init__()
        cfg = encoder.original_encoder.config
        _check_head(cfg, int(projector.weight.shape[1]), int(projector.weight.shape[0]), int(classifier.weight.shape[0]))
        if len(labels) != int(classifier.weight.shape[0]):
            raise ValueError(f"audio classification: {len(labels)} labels for a classifier of {int(classifier.weight.shape[0])} classes")
        self.encoder = encoder
        self.audio_transform = audio_transform
        self.projector = projector
        self.classifier = classifier
        if layer_weights is not None:
            self.layer_weights = layer_weights
        else:
            self.register_parameter("layer_weights", None)
        self.labels = [str(s) for s in labels]

    # ---- host side ----------------------------------------------------------------------------------------------------------------------
    @property
    def sample_rate(self) -> int:
        return int(getattr(self.audio_transform, "sample_rate", 16000))

    @property
    def weighted_layer_sum(self) -> bool:
        return self.layer_weights is not None

    def _weights_stamp(self):
        """Changes whenever a parameter or buffer is written in place, as BaseCTCModule._weights_stamp."""
        epoch = getattr(self.encoder, "_param_epoch", 0)
        ts = self.__dict__.get("_stamp_tensors")
        if ts is None or self.__dict__.get("_stamp_epoch", 0) != epoch:
            ts = self.__dict__["_stamp_tensors"] = list(self.parameters()) + list(self.buffers())
            self.__dict__["_stamp_epoch"] = epoch
        return sum(t._version for t in ts) + (epoch << 48)

    def reset_inference_graphs(self) -> None:
        for k in ("_stamp_tensors", "_graphs", "_packed"):
            self.__dict__.pop(k, None)

    def train(self, mode: bool = True):
        self.reset_inference_graphs()
        return super().train(mode)

    def _apply(self, fn, *args, **kwargs):
        self.reset_inference_graphs()
        self.__dict__.pop("_layer_softmax", None)
        return super()._apply(fn, *args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        self.reset_inference_graphs()
        return super().load_state_dict(*args, **kwargs)

    def _check_forward(self) -> None:
        """The refusals of a forward, by name, before any device work."""
        if self.training or self.encoder.training:
            raise NotImplementedError("audio classification: training mode is not implemented (the classification head has no backward here; "
                                      "fine-tuning classification heads is out of scope); call .eval()")
        if self.weighted_layer_sum and self.encoder.precision == "mxfp8":
            raise NotImplementedError("audio classification: use_weighted_layer_sum under precision='mxfp8' is not enabled: the MX plan does hand out f32 hidden "
                                      "states, but no test bounds the intermediate ones under that mode yet (its accuracy is stated for "
                                      "last_hidden_state only); use precision='bf16' or 'fp32'")

    # ---- device side --------------------------------------------------------------------------------------------------------------------
    def _retire_operands(self) -> None:
        """The head's operands or the soft-max buffer were allocated anew (first use, changed head weights, and after every train() / eval() /
        .to(), which drop them): this module's graphs go, and `operand_epoch` moves so that a graph captured elsewhere with those addresses
        in it (predict_auto's, huggingface/language_bank.py) is retired by its owner's stamp."""
        self.__dict__.pop("_graphs", None)
        self.__dict__["_operand_epoch"] = self.__dict__.get("_operand_epoch", 0) + 1

    @property
    def operand_epoch(self) -> int:
        return self.__dict__.get("_operand_epoch", 0)

    def _refresh(self, device):
        """The head's operands at the encoder's precision and the soft-maxed layer weights, current with the parameters.  Host-issued work
        that a captured graph must not contain: called before a graph is captured or replayed.  The soft-maxed weights live in ONE device
        buffer rewritten in place when `layer_weights` changes, so a captured graph follows it; new head operands retire the graphs."""
        head = [self.projector.weight, self.projector.bias, self.classifier.weight, self.classifier.bias]
        key = (self.encoder.precision, str(device), tuple((t.data_ptr(), t._version) for t in head))
        packed = self.__dict__.get("_packed")
        with torch.no_grad():
            if packed is None or packed[0] != key:
                prec = 0 if self.encoder.precision == "fp32" else 1
                dt = torch.float32 if prec == 0 else torch.bfloat16      # f32 -> bf16 rounds to nearest even, as the plan rounds its weights
                w = lambda t, dtype: t.detach().to(device=device, dtype=dtype).contiguous()
                ops = dict(prec=prec, proj_w=w(head[0], dt), proj_b=w(head[1], torch.float32), cls_w=w(head[2], dt), cls_b=w(head[3], torch.float32))
                packed = self.__dict__["_packed"] = (key, ops)
                self._retire_operands()
            if self.weighted_layer_sum:
                lw = self.layer_weights
                lw_key = (lw.data_ptr(), lw._version)
                buf = self.__dict__.get("_layer_softmax")
                if buf is None or str(buf.device) != str(device) or buf.shape != lw.shape:
                    buf = self.__dict__["_layer_softmax"] = torch.empty(lw.shape, dtype=torch.float32, device=device)
                    self._retire_operands()                          # a new address: graphs captured on the old one are retired
                    self.__dict__.pop("_layer_softmax_key", None)
                if self.__dict__.get("_layer_softmax_key") != lw_key:
                    buf.copy_(torch.softmax(lw.detach().to(device=device, dtype=torch.float32), dim=-1))
                    self.__dict__["_layer_softmax_key"] = lw_key
        return packed[1]

    def _run(self, x: torch.Tensor, lengths: torch.Tensor, class_slot: Optional[torch.Tensor] = None,
             slot: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Front end, encoder, pool and head on the current stream; no host synchronisation.  -> (logits f32 [B, n_labels], top1 int32 [B],
        top1_logp f32 [B]).  class_slot int32 [n_labels] and slot int32 [>= B] (both on the device): the head also writes slot[b], the
        class_slot of the arg-max over the classes whose class_slot is not negative, or -1."""
        L = _lib.lib()
        ops = self.__dict__["_packed"][1]
        device = x.device
        stream = torch.cuda.current_stream(device).cuda_stream
        enc = self.encoder
        b = int(x.shape[0])
        feats, _ = self.audio_transform(x, lengths)
        plan = enc._plan(device)
        plan.bank = enc._bank_for(feats)
        plan.lang_bank = None
        key_len = None
        if enc.mask_input:
            cfg = enc.original_encoder.config
            key_len = feat_extract_output_lengths(cfg.conv_kernel, cfg.conv_stride, lengths.to(device).long()).to(torch.int32).contiguous()
        state: Dict[str, Any] = {}

        def pool(index: int, h: torch.Tensor, w: Optional[torch.Tensor]) -> None:
            if h.dtype != torch.float32 or not h.is_contiguous():
                h = h.to(torch.float32).contiguous()
            bb, t, c = h.shape
            if "partials" not in state:
                state["t"], state["c"] = int(t), int(c)
                state["partials"] = torch.empty(max(int(L.ts_seq_cls_pool_workspace_bytes(bb, t, c)), 16), dtype=torch.uint8, device=device)
            elif (state["t"], state["c"]) != (int(t), int(c)):
                raise RuntimeError(f"audio classification: hidden state {index} has shape {tuple(h.shape)}, the first one had t={state['t']}, c={state['c']}")
            st = L.ts_seq_cls_pool(h.data_ptr(), bb, t, c, key_len.data_ptr() if key_len is not None else None,
                                   w.data_ptr() if w is not None else None, int(index > 0), state["partials"].data_ptr(), stream)
            _lib.check(st, "ts_seq_cls_pool")

        ll = lengths if enc.mask_input else None
        if self.weighted_layer_sum:
            soft = self.__dict__["_layer_softmax"]
            seen = []

            def tap(index: int, h: torch.Tensor) -> None:
                seen.append(index)
                pool(index, h, soft[index: index + 1])
            plan.forward(feats, ll, tap=tap)
            if seen != list(range(int(soft.shape[0]))):
                raise RuntimeError(f"audio classification: the plan tapped hidden states {seen}, layer_weights has {int(soft.shape[0])} entries")
        else:
            pool(0, plan.forward(feats, ll), None)
        p, n = int(ops["proj_w"].shape[0]), int(ops["cls_w"].shape[0])
        ws = torch.empty(max(int(L.ts_seq_cls_head_workspace_bytes(b, p)), 16), dtype=torch.uint8, device=device)
        logits = torch.empty(b, n, dtype=torch.float32, device=device)
        top1 = torch.empty(b, dtype=torch.int32, device=device)
        logp = torch.empty(b, dtype=torch.float32, device=device)
        st = L.ts_seq_cls_head(state["partials"].data_ptr(), b, state["t"], state["c"], ops["proj_w"].data_ptr(), ops["proj_b"].data_ptr(), p,
                               ops["cls_w"].data_ptr(), ops["cls_b"].data_ptr(), n, class_slot.data_ptr() if class_slot is not None else None,
                               ws.data_ptr(), logits.data_ptr(), top1.data_ptr(), logp.data_ptr(), slot.data_ptr() if slot is not None else None,
                               ops["prec"], stream)
        _lib.check(st, "ts_seq_cls_head")
        return logits, top1, logp

    def _prepare(self, x: torch.Tensor) -> torch.Tensor:
        self._check_forward()                                       # by name, before the GPU check
        _t.require_gpu(x, "audio classification")
        x = x.to(torch.float32).contiguous()
        self._refresh(x.device)
        return x

    def _forward_eager(self, x: torch.Tensor, lengths: torch.Tensor):
        x = self._prepare(x)
        with torch.no_grad():
            return self._run(x, lengths)

    def _graphed(self, x: torch.Tensor, lengths: torch.Tensor):
        """_run replayed from a hipGraph per input signature: the graph's OWN output buffers, overwritten by the next call of the signature."""
        from ..utils import GraphedForward
        x = self._prepare(x)                                        # may retire the graphs: before the table is read
        graphs = self.__dict__.get("_graphs")
        key = (self._weights_stamp() - self._layer_weights_version(), self.encoder.precision)
        if graphs is None or graphs[0] != key:
            graphs = self.__dict__["_graphs"] = (key, GraphedForward(lambda xx, ll: self._run(xx, ll)))
        if lengths.device != x.device:
            lengths = lengths.to(x.device)
        return graphs[1](x, lengths)

    def _layer_weights_version(self) -> int:
        # layer_weights reach the graph through the soft-max buffer, rewritten in place: a change of theirs alone retires no graph
        return self.layer_weights._version if self.layer_weights is not None else 0

    def forward(self, x: torch.Tensor, lengths: torch.Tensor) -> torch.Tensor:
        """[batch, time] audio, samples per clip -> f32 logits [batch, n_labels].  A checkpoint trained with an attention mask pools over each
        clip's feature length, any other over all frames -- as transformers does with and without `attention_mask`."""
        return self._forward_eager(x, lengths)[0]

    def _infer(self, x: torch.Tensor):
        lengths = torch.full((x.shape[0],), x.shape[-1], dtype=torch.int32, device=x.device)
        if self.graph_inference and x.is_cuda and not torch.cuda.is_current_stream_capturing():
            return self._graphed(x, lengths)
        return self._forward_eager(x, lengths)

    def predict(self, x: torch.Tensor) -> List[str]:
        """The label of every clip's arg-max class; every clip is treated as full length, like BaseCTCModule.predict."""
        _, top1, _ = self._infer(x)
        return [self.labels[i] for i in top1.tolist()]

    def predict_topk(self, x: torch.Tensor, k: int = 5) -> List[List[Tuple[str, float]]]:
        """Per clip the k most probable labels with their probabilities, the most probable first."""
        k = int(k)
        if k < 1 or k > len(self.labels):
            raise ValueError(f"predict_topk: k must be between 1 and the number of labels ({len(self.labels)}), got {k}")
        logits, _, _ = self._infer(x)
        prob, idx = torch.softmax(logits, dim=-1).topk(k, dim=-1)
        return [[(self.labels[i], float(q)) for i, q in zip(ii, qq)] for ii, qq in zip(idx.tolist(), prob.tolist())]


def classifier_from_huggingface(model, feature_extractor) -> AudioClassifierModule:
    """Assemble the module from already-loaded transformers objects: `model` a `...ForSequenceClassification` of a supported family (the offline
    entry point for randomly initialised models; what load_huggingface_classifier does after its two `from_pretrained` calls).  Refused by name,
    before any device work: whatever the encoder refuses for CTC checkpoints, use_weighted_layer_sum on the conformer and SEW plans, and a
    classifier_proj_size or num_labels beyond the head kernel's limits."""
    for attr in ("projector", "classifier"):
        if not isinstance(getattr(model, attr, None), nn.Linear):
            raise NotImplementedError(f"audio classification: {type(model).__name__} has no `{attr}` Linear (a ...ForSequenceClassification has; the "
                                      "...ForAudioFrameClassification and ...ForXVector heads are out of scope)")
    cfg = model.base_model.config
    if getattr(cfg, "add_adapter", False):
        raise NotImplementedError("audio classification: add_adapter=True (transformers' sequence classification refuses the adapter too)")
    _check_head(cfg, int(model.projector.weight.shape[1]), int(model.projector.weight.shape[0]), int(model.classifier.weight.shape[0]))
    n = int(model.classifier.weight.shape[0])
    id2label = getattr(model.config, "id2label", None) or {}
    labels = [str(id2label.get(i, id2label.get(str(i), f"LABEL_{i}"))) for i in range(n)]
    mask_input = bool(feature_extractor.return_attention_mask)
    audio_transform = Wav2Vec2Preprocess(mask_input=mask_input)
    audio_transform.sample_rate = int(getattr(feature_extractor, "sampling_rate", 16000))
    layer_weights = model.layer_weights if getattr(cfg, "use_weighted_layer_sum", False) else None
    module = AudioClassifierModule(HuggingFaceEncoderAdapt(model.base_model, mask_input=mask_input), audio_transform, model.projector,
                                   model.classifier, labels, layer_weights)
    return module.eval()


def load_huggingface_classifier(model_name: str, **model_kwargs: Dict[str, Any]) -> AudioClassifierModule:
    """`model_name`: hub identifier ("facebook/mms-lid-126"; needs the network) or a local directory written by `save_pretrained`;
    `model_kwargs` go to `AutoModelForAudioClassification.from_pretrained`."""
    from transformers import AutoFeatureExtractor, AutoModelForAudioClassification
    model = AutoModelForAudioClassification.from_pretrained(model_name, **model_kwargs)
    feature_extractor = AutoFeatureExtractor.from_pretrained(model_name)
    return classifier_from_huggingface(model, feature_extractor)
