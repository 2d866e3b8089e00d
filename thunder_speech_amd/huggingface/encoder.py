"""wav2vec2 encoder on the HIP kernels of csrc/w2v_conv.hip, w2v_rows.hip, w2v_posconv.hip and w2v_attn.hip.

The reference hands the whole encoder to transformers (`_HuggingFaceEncoderAdapt.forward`,
src/thunder/huggingface/compatibility.py:31-42: `self.original_encoder(audio, attention_mask=...)`, then
`last_hidden_state.transpose(-1, -2)` and `_get_feat_extract_output_lengths`).  Here the transformers module only OWNS the
weights (same attribute name `original_encoder`, same state-dict keys, so checkpoints and fine-tuning code see no
difference); the arithmetic runs in `Wav2Vec2Plan`, which keeps packed fp32 device copies of the weights and issues one C-ABI
call per stage.  Both published families (group-norm / post-LN: wav2vec2-base-960h, -large-960h; layer-norm / pre-LN: -large-lv60, xlsr);
WavLM runs the same sequence with its gated relative-position attention (csrc/wavlm.hip, include/thunder_speech_amd/wavlm.h) in place of
the wav2vec2 one (fine-tuning in mixed precision only: csrc/wavlm_train.hip); wav2vec2-conformer (rotary) runs conformer blocks behind the same
front end (huggingface/conformer.py; fine-tuning in mixed precision only: huggingface/conformer_train.py, csrc/conformer_train.hip); SEW runs the post-LN layers at 1 / squeeze_factor of the frame rate between csrc/sew.hip's
squeeze and an upsampling GEMM (huggingface/sew.py, include/thunder_speech_amd/sew.h; fine-tuning in mixed precision only: huggingface/sew_train.py, csrc/sew_train.hip); MMS (config.adapter_attn_dim: an attention adapter behind every pre-LN layer) and the head_dim 80
of MMS-1B / XLS-R 1B run on csrc/mms.hip and the head_dim 80 kernel of csrc/w2v_attn.hip (include/thunder_speech_amd/mms.h, inference only); training mode (fine-tuning with the conv feature extractor frozen) runs
through the chain module TRAIN_CHAINS names for the model type (huggingface/train.py, conformer_train.py, sew_train.py); no CPU fallback."""
from __future__ import annotations

import importlib
import math
import os

import ctypes as C
from typing import Dict, Optional, Tuple

import torch
from torch import nn

from .. import _lib, tensors as _t
from ..blocks import _PackedCache

__all__ = ["Wav2Vec2Plan", "HuggingFaceEncoderAdapt", "LoraBank", "feat_extract_output_lengths", "relative_position_bucket", "wavlm_bucket_table"]


def feat_extract_output_lengths(conv_kernel, conv_stride, lengths: torch.Tensor, adapter_layers: int = 0, adapter_stride: int = 2) -> torch.Tensor:
    """transformers' `_get_feat_extract_output_lengths`: floor((len - k) / s) + 1 per conv layer (integer tensor in, out); with an adapter behind the
    encoder (config.add_adapter) also floor((len - 1) / adapter_stride) + 1 per adapter layer."""
    out = lengths
    for k, s in zip(conv_kernel, conv_stride):
        out = torch.div(out - k, s, rounding_mode="floor") + 1
    for _ in range(adapter_layers):
        out = torch.div(out - 1, adapter_stride, rounding_mode="floor") + 1
    return out


# AutoModelForCTC families with a HIP path (the reference loads any of them, huggingface/compatibility.py:77): wav2vec2 (both published
# families), hubert (the same layers; the feature projection's LayerNorm is optional) and data2vec-audio (the reference's own test,
# tests/huggingface/test_module_huggingface.py:107-110: layer-norm conv feature extractor, post-LN encoder, the positional embedding as a
# stack of grouped convs each followed by an affine-free LayerNorm and GELU); unispeech / unispeech-sat (UniSpeechModel / UniSpeechSatModel run the wav2vec2
# encoder arithmetic unchanged: tests/test_oracle_w2v.py checks the oracle against both); wavlm (base / base-plus: group norm, post-LN; large: layer
# norm, pre-LN): the wav2vec2 layers with WavLMAttention's gated relative-position bias in the attention core (csrc/wavlm.hip, head_dim 64 -- every
# published WavLM -- fine-tuned with train_precision="bf16" only, csrc/wavlm_train.hip); wav2vec2-conformer with rotary position embeddings
# (fine-tuned with train_precision="bf16" only, huggingface/conformer_train.py): the wav2vec2 front end and adapter around conformer blocks (huggingface/conformer.py, csrc/conformer.hip,
# include/thunder_speech_amd/conformer.h); sew (fine-tuned with train_precision="bf16" only, huggingface/sew_train.py): wav2vec2's post-LN layers at 1 / squeeze_factor of the frame rate between a
# strided positional conv added to an average pool and an upsampling projection (huggingface/sew.py, csrc/sew.hip, include/thunder_speech_amd/sew.h).
# Others (sew-d's disentangled attention, the conformer's relative-position variant ...) have layers this library holds no kernels for and raise.
# Fine-tuning (huggingface/train.py, TRAINABLE_MODEL_TYPES): every family above but the conformer, which trains on the chain of
# huggingface/conformer_train.py, and sew, which trains on the chain of huggingface/sew_train.py (both in mixed precision only).  hubert, unispeech and unispeech-sat train on the
# wav2vec2 chain (f32 and mixed precision); data2vec-audio on it with one autograd node per layer of its positional stack (PosConvStackLayer,
# csrc/posconv_stack_train.hip, include/thunder_speech_amd/posconv_stack_train.h); wavlm in mixed precision only.
SUPPORTED_MODEL_TYPES = ("wav2vec2", "hubert", "data2vec-audio", "unispeech", "unispeech-sat", "wavlm", "wav2vec2-conformer", "sew")
CONFORMER_ACTIVATIONS = ("swish", "silu", "gelu")
# model_type -> the module of this package that holds its fine-tuning chain: `refuse_untrainable(adapt)` (by name, no device work) and
# `train_forward(adapt, audio, lengths)`.  A new family with a chain of its own is one more entry here
TRAIN_CHAINS = {**{model_type: "train" for model_type in SUPPORTED_MODEL_TYPES}, "wav2vec2-conformer": "conformer_train", "sew": "sew_train"}


def train_chain(model_type: str):
    """The module that fine-tunes `model_type` (imported on first use: the chains import this module).  A type outside the table goes to
    huggingface/train.py, whose `refuse_untrainable` names it."""
    return importlib.import_module("." + TRAIN_CHAINS.get(model_type, "train"), __package__)


def relative_position_bucket(relative_positions: torch.Tensor, num_buckets: int, max_distance: int) -> torch.Tensor:
    """WavLMAttention._relative_positions_bucket (transformers modeling_wavlm.py) restated op for op: the same float32 torch operations in the
    same order, so the bucket boundaries of the log branch fall where transformers puts them (a device logf one ulp away would move some)."""
    num_buckets = num_buckets // 2
    relative_buckets = (relative_positions > 0).to(torch.long) * num_buckets
    relative_positions = torch.abs(relative_positions)
    max_exact = num_buckets // 2
    is_small = relative_positions < max_exact
    if_large = torch.log(relative_positions.float() / max_exact)
    if_large = if_large / math.log(max_distance / max_exact)
    if_large = if_large * (num_buckets - max_exact)
    if_large = (max_exact + if_large).to(torch.long)
    if_large = torch.min(if_large, torch.full_like(if_large, num_buckets - 1))
    relative_buckets += torch.where(is_small, relative_positions, if_large)
    return relative_buckets


def wavlm_bucket_table(num_buckets: int, max_distance: int) -> torch.Tensor:
    """int32 [max_distance + 1]: the bucket of d = -|d| (no sign offset) for 0 <= |d| <= max_distance -- the `abs_bucket` table of ts_wavlm_rel_bias,
    which adds the offset of d > 0 and clamps |d| to max_distance on the device (every |d| >= max_distance lands in bucket num_buckets / 2 - 1)."""
    return relative_position_bucket(-torch.arange(max_distance + 1, dtype=torch.long), num_buckets, max_distance).to(torch.int32)


def _check_conformer_config(cfg, bad: list) -> None:
    """wav2vec2-conformer: the rotary variant at head_dim 64, swish / gelu, odd depthwise kernels up to 63 (csrc/conformer.hip)."""
    pet = getattr(cfg, "position_embeddings_type", None)
    if pet == "relative":
        bad.append("model_type='wav2vec2-conformer' with position_embeddings_type='relative' (the Transformer-XL relative-position attention "
                   "has no HIP kernel; the rotary variant runs)")
    elif pet is None:
        bad.append("model_type='wav2vec2-conformer' with position_embeddings_type=None (a conformer without position embeddings is not a "
                   "published checkpoint; the rotary variant runs)")
    elif pet != "rotary":
        bad.append(f"model_type='wav2vec2-conformer' with position_embeddings_type={pet!r}")
    if int(cfg.hidden_size) != 64 * int(cfg.num_attention_heads):
        bad.append(f"model_type='wav2vec2-conformer' with head_dim={int(cfg.hidden_size) // int(cfg.num_attention_heads)} (the rotary LayerNorm "
                   "kernel takes head_dim 64, as every published conformer)")
    if getattr(cfg, "hidden_act", None) not in CONFORMER_ACTIVATIONS:
        bad.append(f"model_type='wav2vec2-conformer' with hidden_act={getattr(cfg, 'hidden_act', None)!r} (supported: {', '.join(CONFORMER_ACTIVATIONS)})")
    k = int(cfg.conv_depthwise_kernel_size)
    if k < 1 or k > 63 or k % 2 == 0:
        bad.append(f"model_type='wav2vec2-conformer' with conv_depthwise_kernel_size={k} (odd kernels up to 63 run)")
    if getattr(cfg, "feat_extract_activation", "gelu") != "gelu":
        bad.append("feat_extract_activation != gelu")


ATTN_ADAPTER_MAX_DIM = 64          # ts_mms_attn_adapter_fwd: adapter_attn_dim a multiple of 16 up to 64, hidden a multiple of 8 up to 4096


def has_attn_adapters(cfg) -> bool:
    """config.adapter_attn_dim puts a Wav2Vec2AttnAdapterLayer behind every Wav2Vec2EncoderLayerStableLayerNorm (MMS); transformers' post-LN layer
    class has none, whatever the config says."""
    return (getattr(cfg, "adapter_attn_dim", None) is not None and bool(getattr(cfg, "do_stable_layer_norm", False))
            and getattr(cfg, "model_type", "wav2vec2") == "wav2vec2")


def _check_sew_config(cfg, bad: list) -> None:
    """sew: head_dim 64 (the fused attention with key lengths), erf GELU throughout, no adapter (SEWModel has none)."""
    heads, hidden, groups = int(cfg.num_attention_heads), int(cfg.hidden_size), int(cfg.num_conv_pos_embedding_groups)
    if hidden != 64 * heads:
        bad.append(f"model_type='sew' with head_dim={hidden // heads} (the attention kernel with key lengths takes head_dim 64, as every published SEW)")
    if getattr(cfg, "hidden_act", "gelu") != "gelu":
        bad.append(f"model_type='sew' with hidden_act={cfg.hidden_act!r} (gelu runs)")
    if getattr(cfg, "feat_extract_activation", "gelu") != "gelu":
        bad.append(f"model_type='sew' with feat_extract_activation={cfg.feat_extract_activation!r} (gelu runs: the conv feature extractor, the positional "
                   "conv and the upsampler share it)")
    if int(getattr(cfg, "squeeze_factor", 2)) < 1:
        bad.append(f"model_type='sew' with squeeze_factor={cfg.squeeze_factor}")
    if groups < 1 or hidden % groups:
        bad.append(f"model_type='sew' with hidden_size={hidden} not a multiple of num_conv_pos_embedding_groups={groups}")
    if getattr(cfg, "add_adapter", False):
        bad.append("model_type='sew' with add_adapter=True (SEWModel has no adapter)")


def _check_config(cfg) -> None:
    bad = []
    if getattr(cfg, "model_type", "wav2vec2") == "sew-d":
        bad.append(f"model_type='sew-d' (its disentangled attention has no HIP kernel; supported: {', '.join(SUPPORTED_MODEL_TYPES)})")
    elif getattr(cfg, "model_type", "wav2vec2") not in SUPPORTED_MODEL_TYPES:
        bad.append(f"model_type={cfg.model_type!r} (supported: {', '.join(SUPPORTED_MODEL_TYPES)})")
    if getattr(cfg, "conv_pos_batch_norm", False):
        bad.append("conv_pos_batch_norm=True")
    if getattr(cfg, "feat_extract_norm", "group") not in ("group", "layer"):
        bad.append(f"feat_extract_norm={cfg.feat_extract_norm!r}")
    if getattr(cfg, "model_type", "wav2vec2") == "wav2vec2-conformer":
        _check_conformer_config(cfg, bad)
        if bad:
            raise NotImplementedError("wav2vec2-conformer HIP path: unsupported configuration: " + ", ".join(bad))
        return
    if getattr(cfg, "model_type", "wav2vec2") == "sew":
        _check_sew_config(cfg, bad)
        if bad:
            raise NotImplementedError("sew HIP path: unsupported configuration: " + ", ".join(bad))
        return
    if getattr(cfg, "hidden_act", "gelu") != "gelu" or getattr(cfg, "feat_extract_activation", "gelu") != "gelu":
        bad.append("activation != gelu")
    if getattr(cfg, "position_embeddings_type", None) not in (None, "absolute") and hasattr(cfg, "position_embeddings_type"):
        bad.append(f"position_embeddings_type={cfg.position_embeddings_type!r}")
    if getattr(cfg, "model_type", "wav2vec2") == "wavlm" and int(cfg.hidden_size) != 64 * int(cfg.num_attention_heads):
        bad.append(f"model_type='wavlm' with head_dim={int(cfg.hidden_size) // int(cfg.num_attention_heads)} (the gated relative-position attention "
                   "kernels take head_dim 64, as every published WavLM)")
    if has_attn_adapters(cfg):
        a, c = int(cfg.adapter_attn_dim), int(cfg.hidden_size)
        if a < 16 or a % 16 or a > ATTN_ADAPTER_MAX_DIM:
            bad.append(f"adapter_attn_dim={a} (the attention-adapter kernel takes multiples of 16 up to {ATTN_ADAPTER_MAX_DIM}; MMS has 16)")
        elif c % 8 or c > 4096:
            bad.append(f"adapter_attn_dim={a} with hidden_size={c} (the attention-adapter kernel takes a hidden size that is a multiple of 8, up to 4096)")
    if bad:
        raise NotImplementedError("wav2vec2 HIP path: unsupported configuration: " + ", ".join(bad))


# precision="mxfp8": the families that run on Wav2Vec2Plan's own layer loops (pre-LN and post-LN, any head_dim the bf16 mode takes)
MXFP8_MODEL_TYPES = ("wav2vec2", "hubert", "unispeech", "unispeech-sat", "data2vec-audio")


def check_mxfp8_config(cfg) -> None:
    """Whether precision="mxfp8" runs this configuration; NotImplementedError naming the reason otherwise.  No device work: callable without a GPU."""
    mt = getattr(cfg, "model_type", "wav2vec2")
    bad = []
    if mt == "wavlm":
        bad.append("model_type='wavlm' (its gate reads the bf16 rows of the attention's input, which the mode does not keep)")
    elif mt not in MXFP8_MODEL_TYPES:
        bad.append(f"model_type={mt!r} (the MX products exist for the layers of {', '.join(MXFP8_MODEL_TYPES)})")
    if has_attn_adapters(cfg):
        bad.append(f"adapter_attn_dim={cfg.adapter_attn_dim} (the MMS attention adapters multiply bf16 rows)")
    for name in ("hidden_size", "intermediate_size"):
        if int(getattr(cfg, name)) % 128:
            bad.append(f"{name}={int(getattr(cfg, name))} (the MX product contracts in steps of 128; every published checkpoint of the families in "
                       "scope is a multiple)")
    if bad:
        raise NotImplementedError("precision='mxfp8': unsupported configuration: " + ", ".join(bad))


class MxWeight:
    """A weight [n][k] as the packed MX operand ts_mx_gemm_nt loads (ts_mx_pack_w): element fragments and scale fragments."""
    __slots__ = ("frag", "sfrag", "shape")

    def __init__(self, frag, sfrag, n, k):
        self.frag, self.sfrag, self.shape = frag, sfrag, (n, k)


class Wav2Vec2Plan:
    """Packed weights + launch sequence for one set of encoder weights (HF state-dict keys, see oracle/w2v.py).
    precision "fp32": every GEMM in fp32; "bf16": GEMM operands in bf16 (fp32 accumulation, fp32 residual stream /
    normalisations / softmax) -- each launch also writes the bf16 copy its consumer multiplies with; "mxfp8": "bf16" with the four products
    of every transformer layer (q / k / v, out_proj, the two feed-forward linears) on MX operands -- e4m3 elements, one e8m0 scale per 32
    consecutive K elements, f32 accumulation (csrc/mxfp8.hip) -- an opt-in mode with an accuracy cost (profiles/mxfp8_forward.md)."""

    def __init__(self, cfg, sd: Dict[str, torch.Tensor], device, precision: str = "bf16", feature_extractor_only: bool = False):
        """`feature_extractor_only`: pack the conv feature extractor's weights and nothing else -- the plan of the training path's frozen
        front (huggingface/train.py); `forward` is then unavailable, `feature_extractor` works."""
        _check_config(cfg)
        if precision not in ("fp32", "bf16", "mxfp8"):
            raise ValueError(f"precision must be 'fp32', 'bf16' or 'mxfp8', got {precision!r}")
        # a plan of the feature extractor alone runs "mxfp8" as "bf16"; the plans built on this class (conformer, SEW) hold layers of their own
        if precision == "mxfp8" and (not feature_extractor_only or type(self) is not Wav2Vec2Plan):
            check_mxfp8_config(cfg)
        self.prec = 0 if precision == "fp32" else 1
        self.mx = precision == "mxfp8" and not feature_extractor_only
        f = lambda k: sd[k].detach().to(device=device, dtype=torch.float32).contiguous()
        gw = (lambda t: t.to(torch.bfloat16).contiguous()) if self.prec else (lambda t: t.contiguous())     # GEMM operand
        self.device = torch.device(device)
        self.kernels = [int(k) for k in cfg.conv_kernel]
        self.strides = [int(s) for s in cfg.conv_stride]
        self.dims = [int(c) for c in cfg.conv_dim]
        self.hidden = int(cfg.hidden_size)
        self.heads = int(cfg.num_attention_heads)
        self.n_layers = int(cfg.num_hidden_layers)
        self.kpos = int(cfg.num_conv_pos_embeddings)
        self.groups = int(cfg.num_conv_pos_embedding_groups)
        self.eps = float(cfg.layer_norm_eps)
        self.model_type = getattr(cfg, "model_type", "wav2vec2")
        self.d2v = self.model_type == "data2vec-audio"
        self.wavlm = self.model_type == "wavlm"
        # lv60 / xlsr family; Data2VecAudioConvLayer is always conv -> LayerNorm -> GELU and its config carries no feat_extract_norm
        self.layer_norm_convs = self.d2v or getattr(cfg, "feat_extract_norm", "group") == "layer"
        self.stable_ln = bool(getattr(cfg, "do_stable_layer_norm", False))
        # head_dim 80 (MMS-1B, XLS-R 1B) in bf16 mode: ts_mms_attention_fwd; fp32 mode and every other head_dim keep ts_w2v_attention_fwd
        self.mms_attention = bool(self.prec) and self.model_type != "wavlm" and self.hidden == 80 * self.heads
        self.fp_has_ln = bool(getattr(cfg, "feat_proj_layer_norm", True))                  # HubertFeatureProjection
        opt = lambda k: f(k) if k in sd else None
        self.conv_b = [opt(f"feature_extractor.conv_layers.{i}.conv.bias") if getattr(cfg, "conv_bias", False) else None
                       for i in range(len(self.kernels))]
        self.conv_ln = [(f(f"feature_extractor.conv_layers.{i}.layer_norm.weight"), f(f"feature_extractor.conv_layers.{i}.layer_norm.bias"))
                        for i in range(len(self.kernels))] if self.layer_norm_convs else None
        self.w0 = f("feature_extractor.conv_layers.0.conv.weight").reshape(self.dims[0], self.kernels[0]).contiguous()
        self.gn_w = f("feature_extractor.conv_layers.0.layer_norm.weight")       # GroupNorm affine ("group" family)
        self.gn_b = f("feature_extractor.conv_layers.0.layer_norm.bias")
        # [c_out][c_in][k] -> [c_out][k][c_in]: consecutive taps are consecutive K columns of one GEMM
        self.conv_w = [gw(f(f"feature_extractor.conv_layers.{i}.conv.weight").permute(0, 2, 1))
                       for i in range(1, len(self.kernels))]
        self.feature_extractor_only = bool(feature_extractor_only)
        self.layers = []
        self.attn_adapter_keys = []                      # state-dict keys of the attention adapters this plan packed (MMS), in layer order
        if self.feature_extractor_only:
            return
        self._pack_projection(f, gw)
        cg = self.hidden // self.groups
        if self.d2v:
            # Data2VecAudioPositionalConvEmbedding: num_conv_pos_embeddings LAYERS of conv_pos_kernel_size taps, plain weights
            self.pos_layers = int(cfg.num_conv_pos_embeddings)
            self.kpos = int(cfg.conv_pos_kernel_size)
            self.pos_stack = []
            for i in range(self.pos_layers):
                q = f"encoder.pos_conv_embed.layers.{i}.conv."
                self.pos_stack.append((gw(f(q + "weight").view(self.groups, cg, cg, self.kpos).permute(3, 0, 1, 2)), f(q + "bias")))
            self.unit_ln = (torch.ones(self.hidden, device=self.device), torch.zeros(self.hidden, device=self.device))   # elementwise_affine=False
        else:
            # weight_norm(dim=2): w[:, :, j] = g[j] v[:, :, j] / ||v[:, :, j]||
            p = "encoder.pos_conv_embed.conv."
            w_eff = self._weight_normed(sd, f, p)                                             # [C][C/g][k]
            self.pos_w = gw(w_eff.view(self.groups, cg, cg, self.kpos).permute(3, 0, 1, 2))   # [k][g][out][in]
            self.pos_b = f(p + "bias")
        self.enc_ln = (f("encoder.layer_norm.weight"), f("encoder.layer_norm.bias"))
        self._pack_adapter(cfg, sd, f)
        for i in range(self.n_layers):
            q = f"encoder.layers.{i}."
            self.layers.append(self._pack_layer(f, (lambda t: t.contiguous()) if self.mx else gw, q))
            self.layers[-1]["index"] = i                 # the layer's row of a LoRA bank (self.bank)
            if self.mx:
                # the four products' weights: quantised from f32 and packed once; no bf16 copy is kept
                for name in ("wqkv", "wo", "w1", "w2"):
                    self.layers[-1][name] = self._mx_pack(self.layers[-1][name])
            if q + "adapter_layer.linear_1.weight" in sd:
                # Wav2Vec2AttnAdapterLayer (MMS): LayerNorm (eps 1e-5) -> linear_1 [a][c] -> ReLU -> linear_2 [c][a], added to the residual stream
                self.attn_adapter_keys += [q + "adapter_layer." + k for k in ("norm.weight", "norm.bias", "linear_1.weight", "linear_1.bias",
                                                                              "linear_2.weight", "linear_2.bias")]
                self.layers[-1]["ad"] = dict(norm=(f(q + "adapter_layer.norm.weight"), f(q + "adapter_layer.norm.bias")),
                                             w1=gw(f(q + "adapter_layer.linear_1.weight")), b1=f(q + "adapter_layer.linear_1.bias"),
                                             w2=gw(f(q + "adapter_layer.linear_2.weight")), b2=f(q + "adapter_layer.linear_2.bias"))
            if self.wavlm:
                # WavLMAttention's gate: gru_rel_pos_linear [8][64] + bias, gru_rel_pos_const [1][H][1][1] -> [H]
                self.layers[-1].update(gate_w=f(q + "attention.gru_rel_pos_linear.weight"), gate_b=f(q + "attention.gru_rel_pos_linear.bias"),
                                       gate_const=f(q + "attention.gru_rel_pos_const").reshape(-1).contiguous())
        if self.wavlm:
            # the position bias is layer 0's (compute_bias once per forward, reused by every layer): its embedding and the t-independent bucket table
            self.nb, self.md = int(cfg.num_buckets), int(cfg.max_bucket_distance)
            self.rel_embed = f("encoder.layers.0.attention.rel_attn_embed.weight")                      # [num_buckets][H]
            self.abs_bucket = wavlm_bucket_table(self.nb, self.md).to(self.device).contiguous()

    @staticmethod
    def _weight_normed(sd, f, p: str) -> torch.Tensor:
        """The effective weight [C][C/g][k] of the weight_norm(dim=2) conv under the key prefix `p`: w[:, :, j] = g[j] v[:, :, j] / ||v[:, :, j]||."""
        if p + "parametrizations.weight.original0" in sd:
            g, v = f(p + "parametrizations.weight.original0"), f(p + "parametrizations.weight.original1")
        else:
            g, v = f(p + "weight_g"), f(p + "weight_v")
        return g * v / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt()

    @staticmethod
    def _pack_layer(f, gw, q: str) -> dict:
        """The weights of the transformer layer under the key prefix `q` (wav2vec2's names; SEW's layers carry the same ones)."""
        return dict(
            wqkv=gw(torch.cat([f(q + f"attention.{n}_proj.weight") for n in "qkv"], 0)),
            bqkv=torch.cat([f(q + f"attention.{n}_proj.bias") for n in "qkv"], 0).contiguous(),
            wo=gw(f(q + "attention.out_proj.weight")), bo=f(q + "attention.out_proj.bias"),
            ln1=(f(q + "layer_norm.weight"), f(q + "layer_norm.bias")),
            w1=gw(f(q + "feed_forward.intermediate_dense.weight")), b1=f(q + "feed_forward.intermediate_dense.bias"),
            w2=gw(f(q + "feed_forward.output_dense.weight")), b2=f(q + "feed_forward.output_dense.bias"),
            ln2=(f(q + "final_layer_norm.weight"), f(q + "final_layer_norm.bias")))

    def _pack_projection(self, f, gw) -> None:
        """The feature projection: optional LayerNorm (config.layer_norm_eps), then the linear layer -- GEMM operand `gw`."""
        self.fp_ln = (f("feature_projection.layer_norm.weight"), f("feature_projection.layer_norm.bias")) if self.fp_has_ln else None
        self.fp_w, self.fp_b = gw(f("feature_projection.projection.weight")), f("feature_projection.projection.bias")

    def _pack_adapter(self, cfg, sd, f) -> None:
        """Wav2Vec2Adapter behind the encoder (config.add_adapter; Wav2Vec2ConformerAdapter is the same module): optional projection + LayerNorm,
        then strided conv (padding 1, 2x channels) + GLU layers.  Its projection and convolutions run on the f32 GEMM in both precision modes
        (three short layers at an eighth of the frame rate and below)."""
        self.adapter = bool(getattr(cfg, "add_adapter", False))
        if self.adapter:
            self.ad_k, self.ad_s = int(cfg.adapter_kernel_size), int(cfg.adapter_stride)
            self.ad_proj = None
            if "adapter.proj.weight" in sd:
                self.ad_proj = (f("adapter.proj.weight"), f("adapter.proj.bias"), (f("adapter.proj_layer_norm.weight"), f("adapter.proj_layer_norm.bias")))
            self.ad_layers = [(f(f"adapter.layers.{i}.conv.weight").permute(0, 2, 1).contiguous(), f(f"adapter.layers.{i}.conv.bias"))
                              for i in range(int(cfg.num_adapter_layers))]

    def _frag(self, w: torch.Tensor):
        """The bf16 GEMM weight `w` [n][k] in MFMA B-fragment order (ts_gemm_nt_pack_w), packed once per weight: the GEMM kernel then
        loads its B operand from L2 straight into registers.  None in fp32 mode or for shapes the packed kernel does not take."""
        if not self.prec:
            return None
        cache = self.__dict__.setdefault("_frags", {})
        key = w.data_ptr()
        if key not in cache:
            w2 = w.reshape(w.shape[0], -1)
            n, k = w2.shape
            out = None
            if n % 16 == 0 and k % 32 == 0 and w2.is_contiguous():
                out = torch.empty_like(w2)
                st = _lib.lib().ts_gemm_nt_pack_w(w2.data_ptr(), k, n, k, out.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream)
                if st == _lib.TS_EUNSUPPORTED:
                    out = None
                else:
                    _lib.check(st, "ts_gemm_nt_pack_w")
            cache[key] = (out, w)            # holds w so that the key stays unique
        return cache[key][0]

    # ---- a bank of LoRA adaptations (HuggingFaceEncoderAdapt.lora_bank): None, or the LoraBank whose terms follow the attention projections -----
    bank = None

    def _bank_term(self, L, stream, lw, x_op, y, out: bool) -> None:
        """Behind a base product of layer `lw`: y's rows of every clip += the low-rank terms of the slot that clip's id names (one
        ts_lora_bank_fwd; clips with id -1 keep their bits).  out=False: the banked targets among q | k | v on the stacked result y [b][t][3c]
        (the GEMM operand: bf16 in bf16 mode), x_op what the stacked product read; out=True: out_proj on the f32 residual stream y [b][t][c],
        x_op the attention context.  Without a bank, or without a banked target of that kind, no launch."""
        bank = self.bank
        if bank is None:
            return
        targets = tuple(n for n in bank.targets if (n == "out_proj") == out)
        if not targets:
            return
        b, t, c = x_op.shape
        a_bank, b_bank = (bank.a_out, bank.b_out) if out else (bank.a_qkv, bank.b_qkv)
        cols = [0] if out else [c * ("q_proj", "k_proj", "v_proj").index(n) for n in targets]
        cols += [-1] * (3 - len(cols))
        i = lw["index"]
        _lib.check(L.ts_lora_bank_fwd(x_op.data_ptr(), self.prec, c, b, t, c, a_bank[i].data_ptr(), b_bank[i].data_ptr(), bank.scales.data_ptr(),
                                      bank.capacity, len(targets), c, bank.rank, bank.ids.data_ptr(), y.data_ptr(),
                                      0 if out else self.prec, y.shape[-1], cols[0], cols[1], cols[2], stream), "ts_lora_bank_fwd")

    # ---- launch helpers: every helper returns (fp32 result, GEMM operand for the next stage) ------------------------
    def _buf(self, *shape, dtype=torch.float32):
        return torch.empty(*shape, dtype=dtype, device=self.device)

    def _op(self, *shape):
        """Buffer for the GEMM-operand copy of a result (None in fp32 mode: the fp32 result is the operand)."""
        return self._buf(*shape, dtype=torch.bfloat16) if self.prec else None

    @staticmethod
    def _ptr(t):
        return t.data_ptr() if t is not None else None

    def _linear(self, L, stream, x_op, w, bias, act=0, want_op=False, res=None, into=None):
        """want_op: the consumer is another GEMM -- in bf16 mode only the bf16 copy is kept (the fp32 buffer is scratch).
        into: fp32 tensor the product is accumulated into in place (the residual stream; beta = 1 inside the GEMM)."""
        if isinstance(w, MxWeight):
            return self._mx_linear(L, stream, x_op, w, bias, act, want_op, into)
        b, t, k = x_op.shape
        n = w.shape[0]
        y = into if into is not None else self._buf(b, t, n)
        res = into if into is not None else res
        y_op = self._op(b, t, n) if want_op else None
        st = L.ts_w2v_linear_fwd(x_op.data_ptr(), k, w.data_ptr(), self._ptr(bias), self._ptr(res), n, y.data_ptr(), n, self._ptr(y_op),
                                 b * t, n, k, act | (2 if y_op is not None else 0), self.prec, self._ptr(self._frag(w)), stream)
        _lib.check(st, "ts_w2v_linear_fwd")
        return y, (y_op if self.prec else y)

    # ---- precision="mxfp8": an MX operand is the pair (elements uint8 [b][t][k], scales uint8 [b][t][k / 32]) ----------------------------
    def _mx_pack(self, w: torch.Tensor) -> MxWeight:
        """f32 weight [n][k] on the device -> its packed MX operand (quantiser, then the permutation of ts_mx_pack_w)."""
        L = _lib.lib()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        n, k = w.shape
        q, s = self._buf(n, k, dtype=torch.uint8), self._buf(n, k // 32, dtype=torch.uint8)
        _lib.check(L.ts_mx_quantize_rows(w.data_ptr(), 0, k, n, k, q.data_ptr(), k, s.data_ptr(), k // 32, stream), "ts_mx_quantize_rows")
        frag, sfrag = self._buf(n * k, dtype=torch.uint8), self._buf(int(L.ts_mx_pack_w_scale_bytes(n, k)), dtype=torch.uint8)
        _lib.check(L.ts_mx_pack_w(q.data_ptr(), k, s.data_ptr(), k // 32, n, k, frag.data_ptr(), sfrag.data_ptr(), stream), "ts_mx_pack_w")
        return MxWeight(frag, sfrag, n, k)

    def _mx_linear(self, L, stream, x_op, w: MxWeight, bias, act, want_op, into):
        """_linear on MX operands.  x_op: an MX operand, or bf16 rows (the attention context), which are quantised first.  into: accumulated in
        place (f32 residual stream); act=1 with want_op: GELU, result as the next product's MX operand; else bias -> bf16 rows."""
        n, k = w.shape
        if isinstance(x_op, torch.Tensor):
            b, t, _ = x_op.shape
            xq, xs = self._buf(b, t, k, dtype=torch.uint8), self._buf(b, t, k // 32, dtype=torch.uint8)
            _lib.check(L.ts_mx_quantize_rows(x_op.data_ptr(), 1, k, b * t, k, xq.data_ptr(), k, xs.data_ptr(), k // 32, stream), "ts_mx_quantize_rows")
        else:
            xq, xs = x_op
            b, t, _ = xq.shape
        y = y16 = yq = ys = None
        if into is not None:
            ep, y, out = _lib.STAGED["mxfp8"].defines["TS_MX_EP_ACCUM"], into, None
        elif act == 1 and want_op:
            yq, ys = self._buf(b, t, n, dtype=torch.uint8), self._buf(b, t, n // 32, dtype=torch.uint8)
            ep, out = _lib.STAGED["mxfp8"].defines["TS_MX_EP_GELU_MX"], (yq, ys)
        elif act == 0 and want_op:
            y16 = self._buf(b, t, n, dtype=torch.bfloat16)
            ep, out = _lib.STAGED["mxfp8"].defines["TS_MX_EP_BF16"], y16
        else:
            raise NotImplementedError("precision='mxfp8': this product has no MX epilogue")
        _lib.check(L.ts_mx_gemm_nt(xq.data_ptr(), k, xs.data_ptr(), k // 32, w.frag.data_ptr(), w.sfrag.data_ptr(), self._ptr(bias), ep,
                                   self._ptr(y), n, self._ptr(y16), n, self._ptr(yq), n, self._ptr(ys), n // 32, b * t, n, k, stream), "ts_mx_gemm_nt")
        return y, out

    def _mx_ln(self, L, stream, x, wb, res, xbias, want_f32):
        """_ln with the result as an MX operand (and f32 when `want_f32`)."""
        b, t, c = x.shape
        q, s = self._buf(b, t, c, dtype=torch.uint8), self._buf(b, t, c // 32, dtype=torch.uint8)
        y = torch.empty_like(x) if want_f32 else None
        _lib.check(L.ts_mx_layernorm_fwd(x.data_ptr(), self._ptr(res), self._ptr(xbias), wb[0].data_ptr(), wb[1].data_ptr(), self.eps, b * t, c,
                                         self._ptr(y), q.data_ptr(), c, s.data_ptr(), c // 32, stream), "ts_mx_layernorm_fwd")
        return y, (q, s)

    def _ln(self, L, stream, x, wb, res=None, xbias=None, want_op=True, act=0, eps=None, want_f32=True, mx=False):
        """want_f32=False (bf16 mode only): the f32 result has no reader -- only the GEMM-operand copy is written.
        mx (precision="mxfp8": the LayerNorms in front of a layer product): the operand copy is an MX operand."""
        if mx:
            return self._mx_ln(L, stream, x, wb, res, xbias, want_f32)
        y_op = self._op(*x.shape) if want_op else None
        y = torch.empty_like(x) if (want_f32 or y_op is None) else None
        st = L.ts_w2v_layernorm_fwd(x.data_ptr(), self._ptr(res), self._ptr(xbias), wb[0].data_ptr(), wb[1].data_ptr(),
                                    self.eps if eps is None else eps, x.shape[0] * x.shape[1], x.shape[2], act, self._ptr(y),
                                    self._ptr(y_op), stream)
        _lib.check(st, "ts_w2v_layernorm_fwd")
        return y, (y_op if self.prec else y)

    # ---- a bank of MMS languages (BaseCTCModule.language_bank): None, or the LanguageBank whose adapters replace this plan's own, per clip ------
    lang_bank = None

    def _attn_adapter(self, L, stream, h, lw, next_ln, last: bool):
        """h += adapter(h) in place, and LN(h; next_ln) in the same launch: the next layer's layer_norm as the GEMM operand of its QKV product, or
        (`last`) encoder.layer_norm as the f32 result of the encoder.  -> (f32 result or None, GEMM operand or None).  The adapter is layer
        `lw`'s own, or with a language bank the one of each clip's language (ts_mms_lang_bank_adapter_fwd, the same arithmetic)."""
        y = torch.empty_like(h) if (last or not self.prec) else None
        y_op = self._op(*h.shape) if (self.prec and not last) else None
        if self.lang_bank is not None:
            self.lang_bank.adapter(L, stream, h, lw["index"], next_ln, self.eps, y, y_op, self.prec)
            return y, (y_op if self.prec else y)
        ad = lw["ad"]
        a = ad["w1"].shape[0]
        st = L.ts_mms_attn_adapter_fwd(h.data_ptr(), h.shape[0] * h.shape[1], h.shape[2], a, ad["norm"][0].data_ptr(), ad["norm"][1].data_ptr(),
                                       ad["w1"].data_ptr(), ad["b1"].data_ptr(), ad["w2"].data_ptr(), ad["b2"].data_ptr(), next_ln[0].data_ptr(),
                                       next_ln[1].data_ptr(), self.eps, self._ptr(y), self._ptr(y_op), self.prec, stream)
        _lib.check(st, "ts_mms_attn_adapter_fwd")
        return y, (y_op if self.prec else y)

    def feature_extractor(self, audio: torch.Tensor) -> torch.Tensor:
        """[B, n] fp32 -> [B, T', C_last] fp32 (time-major)."""
        return self._feature_extractor(audio)[0]

    def _feature_extractor(self, audio: torch.Tensor, want_op: bool = False):
        """-> (features fp32, their GEMM-operand copy when `want_op`: a feature projection without LayerNorm multiplies them as they are)."""
        L = _lib.lib()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        b, n = audio.shape
        k0, s0, c0 = self.kernels[0], self.strides[0], self.dims[0]
        if n < k0:
            raise RuntimeError(f"wav2vec2: input of {n} samples is shorter than the first conv kernel ({k0})")
        t = (n - k0) // s0 + 1
        ws = self._buf(L.ts_w2v_conv0_workspace_bytes(b, n, c0, k0, s0), dtype=torch.uint8)
        n_conv = len(self.kernels)
        if self.layer_norm_convs:
            # every layer: conv (+ bias) -> LayerNorm over the channels -> GELU; the conv output stays fp32 for the LayerNorm
            h = self._buf(b, t, c0)
            _lib.check(L.ts_w2v_conv0_fwd(audio.data_ptr(), b, n, self.w0.data_ptr(), None, self._ptr(self.conv_b[0]), c0, k0, s0, 1e-5,
                                          h.data_ptr(), None, ws.data_ptr(), stream), "ts_w2v_conv0_fwd")
            h, x_op = self._ln(L, stream, h, self.conv_ln[0], act=1, eps=1e-5, want_op=n_conv > 1 or want_op, want_f32=n_conv == 1)
            for i, w in enumerate(self.conv_w, start=1):
                k, s = self.kernels[i], self.strides[i]
                t_out = (t - k) // s + 1
                if t_out < 1:
                    raise RuntimeError("wav2vec2: input too short for the conv feature extractor")
                y = self._buf(b, t_out, self.dims[i])
                _lib.check(L.ts_w2v_conv_fwd(x_op.data_ptr(), b, t, self.dims[i - 1], w.data_ptr(), self._ptr(self.conv_b[i]), self.dims[i],
                                             k, s, 0, self.prec, y.data_ptr(), None, self._ptr(self._frag(w)), stream), "ts_w2v_conv_fwd")
                h, x_op = self._ln(L, stream, y, self.conv_ln[i], act=1, eps=1e-5, want_op=i < n_conv - 1 or want_op, want_f32=i == n_conv - 1)
                t = t_out
            return h, x_op
        last = n_conv == 1
        h = self._buf(b, t, c0) if (not self.prec or last) else None       # bf16 mode: the next conv only reads the bf16 copy
        h_op = self._op(b, t, c0)
        _lib.check(L.ts_w2v_conv0_fwd(audio.data_ptr(), b, n, self.w0.data_ptr(), self.gn_w.data_ptr(), self.gn_b.data_ptr(), c0, k0,
                                      s0, 1e-5, self._ptr(h), self._ptr(h_op), ws.data_ptr(), stream), "ts_w2v_conv0_fwd")
        x_op = h_op if self.prec else h
        for i, w in enumerate(self.conv_w, start=1):
            k, s = self.kernels[i], self.strides[i]
            t_out = (t - k) // s + 1
            if t_out < 1:
                raise RuntimeError("wav2vec2: input too short for the conv feature extractor")
            last = i == n_conv - 1
            y = self._buf(b, t_out, self.dims[i])
            y_op = None if (last and not want_op) else self._op(b, t_out, self.dims[i])
            _lib.check(L.ts_w2v_conv_fwd(x_op.data_ptr(), b, t, self.dims[i - 1], w.data_ptr(), self._ptr(self.conv_b[i]), self.dims[i], k, s,
                                         1, self.prec, y.data_ptr(), self._ptr(y_op), self._ptr(self._frag(w)), stream), "ts_w2v_conv_fwd")
            h, t = y, t_out
            x_op = y_op if self.prec else y
        return h, x_op

    def forward(self, audio: torch.Tensor, lengths: Optional[torch.Tensor], tap=None) -> torch.Tensor:
        """audio [B, n] fp32 on the GPU; lengths = samples per clip when the model was trained with an attention mask
        (`mask_input`), else None.  Returns last_hidden_state [B, T', C] fp32 (time-major).
        tap: `tap(index, h)` is called, in stream order, with each of transformers' num_hidden_layers + 1 `hidden_states` as an f32 [B, T', C]
        tensor -- post-LN: the output of encoder.layer_norm, then every layer's output; pre-LN: the stream entering layer 0, the un-normalised
        stream after every layer but the last (an MMS adapter is inside its layer), then encoder.layer_norm of the final stream.  The layers
        accumulate into the stream in place: what the tap launches must be issued before it returns (audio classification's weighted layer
        sum, huggingface/classification.py)."""
        if self.feature_extractor_only:
            raise RuntimeError("this Wav2Vec2Plan holds the feature extractor's weights only (feature_extractor_only=True)")
        L = _lib.lib()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        feats, ln_op = self._feature_extractor(audio, want_op=not self.fp_has_ln)
        b, t, _ = feats.shape
        c = self.hidden
        if self.fp_has_ln:
            _, ln_op = self._ln(L, stream, feats, self.fp_ln, want_f32=False)
        h, _ = self._linear(L, stream, ln_op, self.fp_w, self.fp_b)
        key_len = None
        if lengths is not None:
            key_len = feat_extract_output_lengths(self.kernels, self.strides, lengths.to(self.device).long()).to(torch.int32).contiguous()
            _lib.check(L.ts_w2v_mask_rows(h.data_ptr(), b, t, c, key_len.data_ptr(), stream), "ts_w2v_mask_rows")
        ws = self._buf(L.ts_w2v_posconv_workspace_bytes(b, t, c, self.kpos), dtype=torch.uint8)
        hp = torch.empty_like(h)
        if self.d2v:
            # pos = (GELU . LayerNorm_no_affine . conv)^n (h); the encoder's LayerNorm below takes h as its residual: LN(pos + h)
            pos = h
            for w_taps, bias in self.pos_stack:
                _lib.check(L.ts_w2v_groupconv_fwd(pos.data_ptr(), b, t, c, w_taps.data_ptr(), bias.data_ptr(), self.kpos, self.groups, self.prec,
                                                  hp.data_ptr(), ws.data_ptr(), stream), "ts_w2v_groupconv_fwd")
                pos, _ = self._ln(L, stream, hp, self.unit_ln, act=1, eps=1e-5, want_op=False)
            hp, pos_res = pos, h
        else:
            pos_res = None                             # the wav2vec2 / hubert launch adds its input itself: hp = h + gelu(conv(h) + b)
            _lib.check(L.ts_w2v_posconv_fwd(h.data_ptr(), b, t, c, self.pos_w.data_ptr(), self.pos_b.data_ptr(), self.kpos, self.groups,
                                            self.prec, hp.data_ptr(), None, ws.data_ptr(), stream), "ts_w2v_posconv_fwd")
        del ws
        attention = self._attention(L, stream, b, t, key_len)
        if self.stable_ln:
            # pre-LN family: h += attn(LN(h)); h += ffn(LN(h)); one LayerNorm after the last layer
            assert pos_res is None
            h = hp
            y, x_op = None, None                        # LN(h) for what comes next, when the previous layer's adapter launch computed it
            for i, lw in enumerate(self.layers):
                if tap is not None:
                    tap(i, h)                           # the stream entering layer i, before the layer's launches accumulate into it
                if x_op is None:
                    _, x_op = self._ln(L, stream, h, lw["ln1"], want_f32=False, mx=self.mx)
                ctx_op = attention(x_op, lw)
                self._linear(L, stream, ctx_op, lw["wo"], lw["bo"], into=h)                     # h += attn W^T (+ bias in the epilogue)
                self._bank_term(L, stream, lw, ctx_op, h, out=True)
                _, x_op = self._ln(L, stream, h, lw["ln2"], want_f32=False, mx=self.mx)
                _, f1_op = self._linear(L, stream, x_op, lw["w1"], lw["b1"], act=1, want_op=True)
                self._linear(L, stream, f1_op, lw["w2"], lw["b2"], into=h)
                x_op = None
                if "ad" in lw:
                    # MMS: h += adapter(h); the launch also computes the LayerNorm that reads h next -- layer i + 1's, or the encoder's
                    last = i + 1 == len(self.layers)
                    y, x_op = self._attn_adapter(L, stream, h, lw, self.enc_ln if last else self.layers[i + 1]["ln1"], last)
            if self.layers and "ad" in self.layers[-1]:
                h = y
            else:
                h, _ = self._ln(L, stream, h, self.enc_ln, want_op=False)
            if tap is not None:
                tap(len(self.layers), h)
            return self._adapter(L, stream, h) if self.adapter else h
        h, _ = self._post_ln_layers(L, stream, hp, pos_res, attention, tap)
        return self._adapter(L, stream, h) if self.adapter else h

    def _attention(self, L, stream, b, t, key_len):
        """The attention of one layer at `t` frames as a function (x_op, lw) -> context operand, with the workspace (WavLM: and the position bias)
        every layer of this forward shares.  key_len: int32 [B] valid keys per clip on the device, or None."""
        c = self.hidden
        if self.wavlm:
            att_ws =self._buf(L.ts_wavlm_attention_workspace_bytes(b, t, self.heads, self.prec), dtype=torch.uint8)
            rel_bias = self._buf(self.heads, 2 * t - 1)
            _lib.check(L.ts_wavlm_rel_bias(self.rel_embed.data_ptr(), self.abs_bucket.data_ptr(), self.nb, self.md, self.heads, t,
                                           rel_bias.data_ptr(), stream), "ts_wavlm_rel_bias")
        elif self.mms_attention:
            att_ws = None                              # head_dim 80 in bf16 mode: ts_mms_attention_fwd (the fused kernel of csrc/w2v_attn.hip), no [t][t] scores
        else:
            att_ws = self._buf(L.ts_w2v_attention_workspace_bytes(b, t, self.heads, self.prec), dtype=torch.uint8)

        def attention(x_op, lw):
            # x_op: the attention's input as the QKV GEMM reads it -- WavLM's gate is computed from the same rows; lw: the layer's weights
            _, qkv_op = self._linear(L, stream, x_op, lw["wqkv"], lw["bqkv"], want_op=True)
            self._bank_term(L, stream, lw, x_op, qkv_op, out=False)
            ctx_op = self._buf(b, t, c, dtype=torch.bfloat16 if self.prec else torch.float32)
            if self.wavlm:
                _lib.check(L.ts_wavlm_attention_fwd(qkv_op.data_ptr(), b, t, c, self.heads, self._ptr(key_len), self.prec, x_op.data_ptr(), c,
                                                    lw["gate_w"].data_ptr(), lw["gate_b"].data_ptr(), lw["gate_const"].data_ptr(),
                                                    rel_bias.data_ptr(), ctx_op.data_ptr(), att_ws.data_ptr() if att_ws.numel() else None,
                                                    stream), "ts_wavlm_attention_fwd")
                return ctx_op
            if self.mms_attention:
                _lib.check(L.ts_mms_attention_fwd(qkv_op.data_ptr(), b, t, c, self.heads, self._ptr(key_len), ctx_op.data_ptr(), stream),
                           "ts_mms_attention_fwd")
                return ctx_op
            _lib.check(L.ts_w2v_attention_fwd(qkv_op.data_ptr(), b, t, c, self.heads, self._ptr(key_len), self.prec, ctx_op.data_ptr(),
                                              att_ws.data_ptr(), stream), "ts_w2v_attention_fwd")
            return ctx_op

        return attention

    def _post_ln_layers(self, L, stream, hp, pos_res, attention, tap=None):
        """The post-LN family's chain (wav2vec2-base, hubert, data2vec-audio, wavlm-base, SEW at its squeezed frame rate): encoder.layer_norm over
        hp (+ pos_res) before the layers, a LayerNorm after each residual add inside them.  -> (f32 result, its GEMM-operand copy)."""
        h, h_op = self._ln(L, stream, hp, self.enc_ln, res=pos_res, mx=self.mx)
        if tap is not None:
            tap(0, h)
        for i, lw in enumerate(self.layers):
            # the projections accumulate into the residual stream inside the GEMM; their biases ride in the LayerNorm launch
            ctx_op = attention(h_op, lw)
            self._linear(L, stream, ctx_op, lw["wo"], None, into=h)
            self._bank_term(L, stream, lw, ctx_op, h, out=True)
            h, h_op = self._ln(L, stream, h, lw["ln1"], xbias=lw["bo"], mx=self.mx)
            _, f1_op = self._linear(L, stream, h_op, lw["w1"], lw["b1"], act=1, want_op=True)
            self._linear(L, stream, f1_op, lw["w2"], None, into=h)
            h, h_op = self._ln(L, stream, h, lw["ln2"], xbias=lw["b2"], mx=self.mx)
            if tap is not None:
                tap(i + 1, h)
        return h, h_op

    def _adapter(self, L, stream, h: torch.Tensor) -> torch.Tensor:
        """Wav2Vec2Adapter.forward (eval): [B, T, C] -> [B, T'', output_hidden_size]."""
        if self.ad_proj is not None:
            w, bias, ln = self.ad_proj
            b0, t0, c0 = h.shape
            y = self._buf(b0, t0, w.shape[0])
            _lib.check(L.ts_w2v_linear_fwd(h.data_ptr(), c0, w.data_ptr(), bias.data_ptr(), None, w.shape[0], y.data_ptr(), w.shape[0], None,
                                           b0 * t0, w.shape[0], c0, 0, 0, None, stream), "ts_w2v_linear_fwd")       # f32 operands (precision 0)
            h, _ = self._ln(L, stream, y, ln, want_op=False, eps=1e-5)
        b, t, c = h.shape
        for w, bias in self.ad_layers:
            t_pad = t + 2                                          # Conv1d(padding = 1)
            t_out = (t_pad - self.ad_k) // self.ad_s + 1
            if t_out < 1:
                raise RuntimeError("wav2vec2: input too short for the adapter layers")
            hp = self._buf(b, t_pad, c)
            _lib.check(L.ts_w2v_pad_rows(h.data_ptr(), hp.data_ptr(), b, t, t_pad, 1, c, 0, stream), "ts_w2v_pad_rows")
            y = self._buf(b, t_out, 2 * c)
            _lib.check(L.ts_w2v_conv_fwd(hp.data_ptr(), b, t_pad, c, w.data_ptr(), bias.data_ptr(), 2 * c, self.ad_k, self.ad_s, 0, 0, y.data_ptr(),
                                         None, None, stream), "ts_w2v_conv_fwd")
            h = self._buf(b, t_out, c)
            _lib.check(L.ts_w2v_glu_fwd(y.data_ptr(), b * t_out, c, h.data_ptr(), None, stream), "ts_w2v_glu_fwd")
            t = t_out
        return h


LORA_BANK_MAX_CLIPS = 4096         # entries of a bank's id buffer: the largest batch a forward with a bank takes


class LoraBank:
    """The tensors of HuggingFaceEncoderAdapt.lora_bank(): `capacity` slots of LoRA pairs for every layer and target, next to one frozen base
    (include_staged/thunder_speech_amd/queued/lora_bank.h).  Plain tensors at fixed addresses: adding, removing and selecting write in place, so a
    captured graph that read them keeps serving.  a_qkv [layers][capacity][targets among q, k, v][rank][c], b_qkv [...][c][rank], a_out / b_out the
    same with one target (out_proj); `dtype` is the GEMM operands' (bf16 under precision="bf16", f32 under "fp32"); scales f32 [capacity]
    (alpha / rank per slot); ids int32 [LORA_BANK_MAX_CLIPS]: the slot of clip b, -1 = the base alone."""

    def __init__(self, n_layers: int, hidden: int, rank: int, alpha_default: float, targets, capacity: int, precision: str, device):
        self.n_layers, self.hidden, self.rank, self.alpha_default, self.targets, self.capacity = n_layers, hidden, rank, alpha_default, targets, capacity
        self.precision = precision
        self.dtype = torch.float32 if precision == "fp32" else torch.bfloat16
        self.qkv_targets = tuple(t for t in targets if t != "out_proj")
        self.has_out = "out_proj" in targets
        z = lambda *shape: torch.zeros(*shape, dtype=self.dtype, device=device)
        nq = len(self.qkv_targets)
        self.a_qkv = z(n_layers, capacity, nq, rank, hidden) if nq else None
        self.b_qkv = z(n_layers, capacity, nq, hidden, rank) if nq else None
        self.a_out = z(n_layers, capacity, 1, rank, hidden) if self.has_out else None
        self.b_out = z(n_layers, capacity, 1, hidden, rank) if self.has_out else None
        self.scales = torch.zeros(capacity, dtype=torch.float32, device=device)
        self.ids = torch.full((LORA_BANK_MAX_CLIPS,), -1, dtype=torch.int32, device=device)
        self.names = [None] * capacity                   # slot -> name
        self.selection = []                              # what select_adapters() was last given: a name or None per clip

    _TENSORS = ("a_qkv", "b_qkv", "a_out", "b_out", "scales", "ids")

    @property
    def device(self):
        return self.ids.device

    def to(self, device) -> None:
        """Move the tensors (new addresses: the caller retires the graphs captured on the old ones)."""
        for name in self._TENSORS:
            if getattr(self, name) is not None:
                setattr(self, name, getattr(self, name).to(device))

    def pair(self, layer: int, slot: int, target: str):
        """(A [rank][c], B [c][rank]): views into the bank's tensors."""
        if target == "out_proj":
            return self.a_out[layer, slot, 0], self.b_out[layer, slot, 0]
        j = self.qkv_targets.index(target)
        return self.a_qkv[layer, slot, j], self.b_qkv[layer, slot, j]

    def write_ids(self) -> None:
        """The id buffer from `selection`: the slots of the given clips, -1 for a None and for every entry beyond them.  One host-to-device copy at
        a fixed address."""
        host = torch.full((LORA_BANK_MAX_CLIPS,), -1, dtype=torch.int32)
        for i, name in enumerate(self.selection):
            if name is not None:
                host[i] = self.names.index(name)
        self.ids.copy_(host)


class HuggingFaceEncoderAdapt(nn.Module):
    """Same constructor, attributes and return convention as the reference's `_HuggingFaceEncoderAdapt`
    (huggingface/compatibility.py:23-42): `(audio [B, n], lengths) -> (features [B, C, T'], lengths')`."""

    def __init__(self, encoder, mask_input: bool = False, precision: str = "bf16", train_precision: str = "fp32"):
        if train_precision not in ("fp32", "bf16"):
            raise ValueError(f"train_precision must be 'fp32' or 'bf16', got {train_precision!r}")
        super().__init__()
        self.precision = precision
        # arithmetic of the TRAINABLE part in train mode (huggingface/train.py): "fp32" = the reference's, "bf16" = mixed precision (bf16 operands in the
        # linear layers' three products, everything else f32) -- the reference under Lightning's precision="bf16-mixed"
        self.train_precision = train_precision
        self.original_encoder = encoder
        if hasattr(self.original_encoder, "freeze_feature_encoder"):
            self.original_encoder.freeze_feature_encoder()
        elif hasattr(getattr(self.original_encoder, "feature_extractor", None), "_freeze_parameters"):
            # HubertModel and UniSpeechSatModel have no freeze_feature_encoder (only their ForCTC wrappers do), so the reference leaves their conv
            # feature extractor trainable.  The training path here has no backward for those convolutions and refuses an unfrozen one by name:
            # freeze it the way freeze_feature_encoder would, so that .train() works on a loaded checkpoint of either family
            self.original_encoder.feature_extractor._freeze_parameters()
        self.mask_input = mask_input
        self._cache = _PackedCache()
        _check_config(encoder.config)
        if precision == "mxfp8":
            check_mxfp8_config(encoder.config)

    @property
    def precision(self) -> str:
        """"fp32", "bf16" or "mxfp8" (Wav2Vec2Plan).  Assigning another value on a loaded module re-packs the plan on the next forward and, through
        `_param_epoch` (BaseCTCModule._weights_stamp), retires the inference graphs captured with the old one."""
        d = self.__dict__
        return d["_precision"] if "_precision" in d else d["precision"]      # "precision": an adapter unpickled from before this was a property

    @precision.setter
    def precision(self, value: str) -> None:
        if value != self.__dict__.get("_precision"):
            self.__dict__["_precision"] = value
            self.__dict__["_param_epoch"] = self.__dict__.get("_param_epoch", 0) + 1

    def _plan(self, device) -> Wav2Vec2Plan:
        params = list(self.original_encoder.parameters())
        cfg = self.original_encoder.config
        if self.precision == "mxfp8":
            check_mxfp8_config(cfg)                  # by name, before any plan of another family is built
        if getattr(self, "_cache_precision", None) != self.precision:
            # the precision is part of the cache key: flipping `encoder.precision` on a loaded module re-packs the weights
            self._cache, self._cache_precision = _PackedCache(), self.precision
        if getattr(cfg, "model_type", "wav2vec2") == "wav2vec2-conformer":
            from .conformer import ConformerPlan
            # the plan folds running_mean / running_var into bn_scale / bn_shift: a train-mode forward changes those buffers without touching a
            # parameter (no optimizer step), so they belong to the key
            params += [buf for layer in self.original_encoder.encoder.layers
                       for buf in (layer.conv_module.batch_norm.running_mean, layer.conv_module.batch_norm.running_var) if buf is not None]
            return self._cache.get(params, lambda: ConformerPlan(cfg, self.original_encoder.state_dict(), device, self.precision))
        if getattr(cfg, "model_type", "wav2vec2") == "sew":
            from .sew import SEWPlan
            return self._cache.get(params, lambda: SEWPlan(cfg, self.original_encoder.state_dict(), device, self.precision))
        if getattr(self, "lora", None) is not None:
            # eval with unmerged LoRA (a validation step during training): the plan is packed from the effective weights W + s B A, formed with
            # merge_lora()'s f32 operations, and keyed on A and B too, so an optimizer step on them re-packs it
            params += list(self.lora.parameters())

            def build():
                sd = dict(self.original_encoder.state_dict())
                for i, target, _ in self._lora_items():
                    sd[f"encoder.layers.{i}.attention.{target}.weight"] = self._lora_effective(i, target)
                return Wav2Vec2Plan(cfg, sd, device, self.precision)
            return self._cache.get(params, build)
        return self._cache.get(params, lambda: Wav2Vec2Plan(cfg, self.original_encoder.state_dict(), device, self.precision))

    # ------------------------------------------------------------------------------------------------------------------
    # Low-rank adaptation (LoRA, Hu et al. 2021) of the attention projections on a frozen base (no reference counterpart): per layer and target
    # y = x W^T + b + (alpha / rank) (x A^T) B^T with A [rank][in], B [out][rank] trainable.  Train mode (train_precision="bf16" only) keeps the
    # two paths apart (huggingface/train.py LoRALinear, csrc/lora_train.hip): the low-rank term is a product of its own at f32 accumulation, never
    # folded into the bf16 copy of W, where a small B would vanish in the rounding.  Eval mode runs the inference plan on the merged weight
    # W + s B A (f32), which precision="bf16" rounds to bf16 as it rounds every weight: train and eval outputs differ by that rounding.
    def _lora_items(self):
        """(layer index, target name, {lora_A, lora_B}) of every LoRA pair, in layer order."""
        return [(i, target, pair) for i, layer in enumerate(self.lora.layers) for target, pair in layer.items()]

    def _lora_effective(self, i: int, target: str) -> torch.Tensor:
        """W + s B A of one target in f32: what merge_lora() writes and what the eval-mode plan packs (the same operations: bit-equal)."""
        pair = self.lora.layers[i][target]
        w = getattr(self.original_encoder.encoder.layers[i].attention, target).weight
        with torch.no_grad():
            return w.detach().float() + self.lora_scale * (pair["lora_B"].detach().float() @ pair["lora_A"].detach().float())

    def lora_finetuning(self, rank: int = 8, alpha: float = 16.0, targets=("q_proj", "v_proj")) -> Dict[str, nn.Parameter]:
        """Put the encoder into the LoRA fine-tuning regime: every encoder parameter is frozen, and per transformer layer and target projection
        (`targets`: any of q_proj, k_proj, v_proj, out_proj) a pair lora_A [rank][in] (kaiming_uniform_, a = sqrt(5)) / lora_B [out][rank] (zeros) is
        created on this module, so that `state_dict()` and the module's `configure_optimizers` see them.  Returns them, {name: parameter}, named as in
        `state_dict()` (`lora.layers.{i}.{target}.lora_A` / `.lora_B`); hand them and the CTC head (the module's `decoder`) to the optimizer.
        Train mode then runs huggingface/train.py with LoRALinear in place of the target products (train_precision="bf16" only); with any base
        parameter trainable it refuses by name.  wav2vec2-conformer, sew and MMS (adapter_attn_dim) checkpoints are refused by name."""
        from .train import LORA_RANKS, LORA_TARGETS, refuse_lora
        if getattr(self, "lora", None) is not None:
            raise RuntimeError("lora_finetuning: this encoder already carries LoRA parameters (merge_lora() folds them into the base)")
        if getattr(self, "_lora_bank", None) is not None:
            raise RuntimeError("lora_finetuning: this encoder serves a LoRA bank (lora_bank); fine-tune on a copy without one and add the "
                               "result with lora_bank_add()")
        if isinstance(rank, bool) or not isinstance(rank, int) or rank not in LORA_RANKS:
            raise ValueError(f"lora_finetuning: rank must be one of {LORA_RANKS} (the low-rank kernels' widths), got {rank!r}")
        targets = (targets,) if isinstance(targets, str) else tuple(targets)
        bad = [t for t in targets if t not in LORA_TARGETS]
        if bad or not targets or len(set(targets)) != len(targets):
            raise ValueError(f"lora_finetuning: targets must be distinct names out of {LORA_TARGETS}, got {targets!r}")
        if not float(alpha) > 0.0:
            raise ValueError(f"lora_finetuning: alpha must be positive, got {alpha!r}")
        enc = self.original_encoder
        refuse_lora(enc.config)
        for p in enc.parameters():
            p.requires_grad_(False)
        layers = nn.ModuleList()
        for layer in enc.encoder.layers:
            pairs = nn.ModuleDict()
            for target in (t for t in LORA_TARGETS if t in targets):                 # a fixed order, whatever the caller's
                w = getattr(layer.attention, target).weight
                a = torch.empty(rank, w.shape[1], dtype=torch.float32, device=w.device)
                nn.init.kaiming_uniform_(a, a=math.sqrt(5))
                pairs[target] = nn.ParameterDict({"lora_A": nn.Parameter(a),
                                                  "lora_B": nn.Parameter(torch.zeros(w.shape[0], rank, dtype=torch.float32, device=w.device))})
            layers.append(pairs)
        self.lora = nn.ModuleDict({"layers": layers})
        self.lora_rank, self.lora_alpha, self.lora_scale = int(rank), float(alpha), float(alpha) / int(rank)
        self._param_epoch = getattr(self, "_param_epoch", 0) + 1       # BaseCTCModule._weights_stamp: the set of parameters changed
        return {"lora." + n: p for n, p in self.lora.named_parameters()}

    def merge_lora(self) -> None:
        """Fold W += s B A into the base weights (f32) and remove the LoRA parameters; the base stays frozen as it is.  Eval-mode outputs before
        and after are bit-equal: the unmerged plan is packed from the same f32 sums."""
        if getattr(self, "lora", None) is None:
            raise RuntimeError("merge_lora: this encoder carries no LoRA parameters (lora_finetuning() creates them)")
        with torch.no_grad():
            for i, target, _ in self._lora_items():
                w = getattr(self.original_encoder.encoder.layers[i].attention, target).weight
                w.copy_(self._lora_effective(i, target).to(w.dtype))
        del self.lora
        del self.lora_rank, self.lora_alpha, self.lora_scale
        self._param_epoch = getattr(self, "_param_epoch", 0) + 1

    def lora_state_dict(self) -> Dict[str, torch.Tensor]:
        """The LoRA tensors alone ({`lora.layers.{i}.{target}.lora_A` / `.lora_B`: tensor}, detached copies): an adaptation ships without the base."""
        if getattr(self, "lora", None) is None:
            raise RuntimeError("lora_state_dict: this encoder carries no LoRA parameters (lora_finetuning() creates them)")
        return {"lora." + n: p.detach().clone() for n, p in self.lora.named_parameters()}

    def load_lora_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        """Load what lora_state_dict() returned into the parameters lora_finetuning() created (same rank and targets: the keys and shapes must match)."""
        if getattr(self, "lora", None) is None:
            raise RuntimeError("load_lora_state_dict: call lora_finetuning() with the adaptation's rank, alpha and targets first")
        mine = {"lora." + n: p for n, p in self.lora.named_parameters()}
        if set(sd) != set(mine):
            raise KeyError(f"load_lora_state_dict: keys differ (missing {sorted(set(mine) - set(sd))[:3]}, unexpected {sorted(set(sd) - set(mine))[:3]})")
        for n, p in mine.items():
            if tuple(sd[n].shape) != tuple(p.shape):
                raise ValueError(f"load_lora_state_dict: {n} has shape {tuple(sd[n].shape)}, expected {tuple(p.shape)}")
        with torch.no_grad():
            for n, p in mine.items():
                p.copy_(sd[n])

    # ------------------------------------------------------------------------------------------------------------------
    # Serving many adaptations on one base (no reference counterpart): a bank of LoRA pairs next to the frozen, packed base; every clip of a batch
    # picks its pair by name.  Eval mode then runs the base products as they are and adds each clip's low-rank term behind them
    # (Wav2Vec2Plan._bank_term, csrc/lora_bank.hip) with the arithmetic of the training forward -- not the merged weight of `_plan` above, which
    # serves one adaptation per packed copy of the base.  The bank's tensors are plain attributes (no Parameters, no buffers: state_dict() does
    # not change); adding, removing and selecting write at fixed addresses, so captured graphs keep replaying.
    def _bank(self, what: str) -> LoraBank:
        bank = getattr(self, "_lora_bank", None)
        if bank is None:
            raise RuntimeError(f"{what}: this encoder has no LoRA bank (lora_bank() creates one)")
        return bank

    def lora_bank(self, rank: int = 8, alpha_default: float = 16.0, targets=("q_proj", "v_proj"), capacity: int = 8) -> None:
        """Create an empty bank of `capacity` slots for adaptations of rank `rank` on `targets` (ordered as LORA_TARGETS, whatever the caller's
        order); `alpha_default` is the alpha of an adaptation added without one.  The selection starts as the base alone for every clip.
        Refused by name: what lora_finetuning() refuses (conformer, sew, attention adapters), precision="mxfp8", an encoder that carries LoRA
        parameters, a second bank."""
        from .train import LORA_RANKS, LORA_TARGETS, refuse_lora
        if isinstance(rank, bool) or not isinstance(rank, int) or rank not in LORA_RANKS:
            raise ValueError(f"lora_bank: rank must be one of {LORA_RANKS} (the low-rank kernels' widths), got {rank!r}")
        targets = (targets,) if isinstance(targets, str) else tuple(targets)
        bad = [t for t in targets if t not in LORA_TARGETS]
        if bad or not targets or len(set(targets)) != len(targets):
            raise ValueError(f"lora_bank: targets must be distinct names out of {LORA_TARGETS}, got {targets!r}")
        if not float(alpha_default) > 0.0:
            raise ValueError(f"lora_bank: alpha_default must be positive, got {alpha_default!r}")
        if isinstance(capacity, bool) or not isinstance(capacity, int) or capacity < 1:
            raise ValueError(f"lora_bank: capacity must be a positive number of slots, got {capacity!r}")
        enc = self.original_encoder
        refuse_lora(enc.config)
        if self.precision == "mxfp8":
            raise NotImplementedError("lora_bank: a LoRA bank under precision='mxfp8' is not implemented (the low-rank term multiplies the bf16 rows "
                                      "of the LayerNorm, which the mode does not keep next to the MX operand); use precision='bf16' or 'fp32'")
        if getattr(self, "lora", None) is not None:
            raise RuntimeError("lora_bank: this encoder carries LoRA parameters (lora_finetuning); merge_lora() them into the base, or export them "
                               "with lora_state_dict() and add them to the bank of an encoder without them")
        if getattr(self, "_lora_bank", None) is not None:
            raise RuntimeError("lora_bank: this encoder already has a LoRA bank (one bank per encoder; lora_bank_add() fills its slots)")
        device = next(enc.parameters()).device
        self._lora_bank = LoraBank(int(enc.config.num_hidden_layers), int(enc.config.hidden_size), rank, float(alpha_default),
                                   tuple(t for t in LORA_TARGETS if t in targets), capacity, self.precision, device)
        self._param_epoch = getattr(self, "_param_epoch", 0) + 1       # graphs of the bank-less launch sequence are retired

    def lora_bank_names(self):
        """The names of the adaptations in the bank, in slot order."""
        return [n for n in self._bank("lora_bank_names").names if n is not None]

    def lora_bank_add(self, name: str, lora_sd: Dict[str, torch.Tensor], alpha: Optional[float] = None) -> int:
        """Put the adaptation `lora_sd` (what lora_state_dict() returned: the bank's rank and targets) under `name` into a free slot; `alpha`: its
        alpha (default: the bank's alpha_default).  Returns the slot.  Written in place: captured graphs stay valid."""
        bank = self._bank("lora_bank_add")
        if not isinstance(name, str) or not name:
            raise ValueError(f"lora_bank_add: the name must be a non-empty string, got {name!r}")
        if name in bank.names:
            raise RuntimeError(f"lora_bank_add: the bank already holds an adaptation named {name!r} (lora_bank_remove() it first)")
        if None not in bank.names:
            raise RuntimeError(f"lora_bank_add: the bank is full ({bank.capacity} slots: {', '.join(bank.names)}); lora_bank_remove() frees one")
        alpha = bank.alpha_default if alpha is None else float(alpha)
        if not alpha > 0.0:
            raise ValueError(f"lora_bank_add: alpha must be positive, got {alpha!r}")
        c, r = bank.hidden, bank.rank
        want = {f"lora.layers.{i}.{t}.lora_{m}": ((r, c) if m == "A" else (c, r)) for i in range(bank.n_layers) for t in bank.targets for m in "AB"}
        if set(lora_sd) != set(want):
            raise KeyError(f"lora_bank_add: keys differ (missing {sorted(set(want) - set(lora_sd))[:3]}, unexpected {sorted(set(lora_sd) - set(want))[:3]})")
        for n, shape in want.items():
            if tuple(lora_sd[n].shape) != shape:
                raise ValueError(f"lora_bank_add: {n} has shape {tuple(lora_sd[n].shape)}, expected {shape}")
        slot = bank.names.index(None)
        with torch.no_grad():
            for i in range(bank.n_layers):
                for t in bank.targets:
                    a, b = bank.pair(i, slot, t)
                    a.copy_(lora_sd[f"lora.layers.{i}.{t}.lora_A"].detach().to(torch.float32))
                    b.copy_(lora_sd[f"lora.layers.{i}.{t}.lora_B"].detach().to(torch.float32))
            bank.scales[slot] = alpha / r
        bank.names[slot] = name
        return slot

    def lora_bank_remove(self, name: str) -> None:
        """Zero and free the slot of the adaptation `name`; clips that selected it go back to the base alone."""
        bank = self._bank("lora_bank_remove")
        if name not in bank.names:
            raise KeyError(f"lora_bank_remove: no adaptation named {name!r} in the bank (it holds: {', '.join(self.lora_bank_names()) or 'none'})")
        slot = bank.names.index(name)
        bank.names[slot] = None
        if name in bank.selection:
            bank.selection = [None if n == name else n for n in bank.selection]
            bank.write_ids()
        with torch.no_grad():
            for t in (bank.a_qkv, bank.b_qkv, bank.a_out, bank.b_out):
                if t is not None:
                    t[:, slot].zero_()
            bank.scales[slot] = 0.0

    def select_adapters(self, names) -> None:
        """One entry per clip of the batches to come: the name of an adaptation in the bank, or None for the base alone; clips beyond the given
        entries run the base alone.  A host-to-device copy into the bank's id buffer: nothing is re-captured."""
        bank = self._bank("select_adapters")
        names = list(names)
        if len(names) > LORA_BANK_MAX_CLIPS:
            raise ValueError(f"select_adapters: {len(names)} entries; the bank's id buffer holds {LORA_BANK_MAX_CLIPS} clips")
        for n in names:
            if n is not None and n not in bank.names:
                raise KeyError(f"select_adapters: no adaptation named {n!r} in the bank (it holds: {', '.join(self.lora_bank_names()) or 'none'})")
        bank.selection = names
        bank.write_ids()

    def selected_adapters(self):
        """What select_adapters() was last given (a copy; [] after lora_bank())."""
        return list(self._bank("selected_adapters").selection)

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        bank = self.__dict__.get("_lora_bank")
        if bank is not None:
            # .to(device) / .cuda(): the bank follows the base (its dtype is the operands' and stays)
            device = next(self.original_encoder.parameters()).device
            if bank.device != device:
                bank.to(device)
                self._param_epoch = getattr(self, "_param_epoch", 0) + 1
        lang_bank = self.__dict__.get("_language_bank")
        if lang_bank is not None:
            # the language bank (BaseCTCModule.language_bank) follows the base the same way
            device = next(self.original_encoder.parameters()).device
            if lang_bank.device != device:
                lang_bank.to(device)
                self._param_epoch = getattr(self, "_param_epoch", 0) + 1
        return out

    def _bank_for(self, x: torch.Tensor, check_only: bool = False) -> Optional[LoraBank]:
        """The bank an eval forward of the batch `x` runs with (None: no bank), on x's device.  check_only: the refusals alone, no device work."""
        bank = getattr(self, "_lora_bank", None)
        if bank is None:
            return None
        if bank.precision != self.precision:
            raise RuntimeError(f"lora_bank: the bank was created under precision={bank.precision!r} and holds operands of that mode; the encoder now "
                               f"runs precision={self.precision!r}.  Set the precision before lora_bank()")
        if x.shape[0] > LORA_BANK_MAX_CLIPS:
            raise RuntimeError(f"lora_bank: a batch of {x.shape[0]} clips; a forward with a LoRA bank takes up to {LORA_BANK_MAX_CLIPS} (the bank's id buffer)")
        if bank.device != x.device and not check_only:
            bank.to(x.device)                                              # new addresses: retire the graphs captured on the old ones
            self._param_epoch = getattr(self, "_param_epoch", 0) + 1
        return bank

    def _plan_frozen(self, device) -> Wav2Vec2Plan:
        """The plan the training path runs the frozen conv feature extractor on: built from and keyed on the feature extractor's parameters
        only, so an optimizer step on the transformer re-packs nothing and no transformer weight gets a device copy it never uses.  It runs
        at `self.precision` -- with the default "bf16" the FROZEN convolutions multiply bf16 operands (f32 accumulation) while everything
        trainable behind them is f32; pass precision="fp32" for f32 arithmetic throughout (what the parity tests use)."""
        if not hasattr(self, "_fe_cache") or getattr(self, "_fe_cache_precision", None) != self.precision:
            self._fe_cache, self._fe_cache_precision = _PackedCache(), self.precision        # keyed on the precision, as `_plan`'s cache
        fe = self.original_encoder.feature_extractor
        params = list(fe.parameters())
        sd = {"feature_extractor." + k: v for k, v in fe.state_dict().items()}
        return self._fe_cache.get(params, lambda: Wav2Vec2Plan(self.original_encoder.config, sd, device, self.precision, feature_extractor_only=True))

    def adapter_finetuning(self, init: bool = False) -> Dict[str, nn.Parameter]:
        """Put an MMS checkpoint (config.adapter_attn_dim) into the adapter-only fine-tuning regime, transformers' recipe for a new language:
        `init=True` re-initialises the attention adapters (the encoder's own `init_adapter_layers()`, and its Linear / LayerNorm initialisation
        for the adapters' children, which that call does not reach), every encoder parameter is frozen and the
        adapter layers' parameters are made trainable.  Returns those, {name: parameter}, named as in `state_dict()` (under `original_encoder.`);
        hand them and the CTC head (the module's `decoder`) to the optimizer.  Train mode then runs huggingface/train.py with the fused adapter
        node; with any base parameter trainable it refuses by name."""
        enc = self.original_encoder
        if not has_attn_adapters(enc.config):
            raise ValueError("adapter_finetuning: the checkpoint has no attention adapters (config.adapter_attn_dim is None, or the layers are post-LN)")
        if init:
            enc.init_adapter_layers()
            # transformers hands each Wav2Vec2AttnAdapterLayer itself to _init_weights, which knows Linear and LayerNorm but not that container: its
            # children keep their values.  Give them what _init_weights gives those two types, so that a new language starts from fresh adapters
            with torch.no_grad():
                for layer in enc.encoder.layers:
                    ad = layer.adapter_layer
                    for lin in (ad.linear_1, ad.linear_2):
                        lin.weight.normal_(mean=0.0, std=float(enc.config.initializer_range))
                        lin.bias.zero_()
                    ad.norm.weight.fill_(1.0)
                    ad.norm.bias.zero_()
        for p in enc.parameters():
            p.requires_grad_(False)
        out = {}
        for name, p in enc.named_parameters():
            if ".adapter_layer." in name:
                p.requires_grad_(True)
                out["original_encoder." + name] = p
        return out

    def forward(self, audio: torch.Tensor, audio_lengths: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        lang_bank = self.__dict__.get("_language_bank")
        if self.training and lang_bank is not None:
            raise NotImplementedError("wav2vec2 encoder: training with a language bank (BaseCTCModule.language_bank) is not implemented")
        if self.training:
            # fine-tuning (module.py:102-127 through this adapter): transformers' training-mode forward -- frozen conv feature extractor, time
            # masking, dropouts, LayerDrop -- as a chain of autograd nodes on the HIP kernels.  What the family's chain has no backward for
            # (a train_precision, LoRA outside its regime, an adapter, mask_feature_prob, an unfrozen feature extractor ...) is refused by
            # name, before any device work
            chain = train_chain(getattr(self.original_encoder.config, "model_type", "wav2vec2"))
            chain.refuse_untrainable(self)
        else:
            self._bank_for(audio, check_only=True)       # a bank's refusals, by name, before any device work
        _t.require_gpu(audio, "wav2vec2 encoder")
        x = audio.to(torch.float32).contiguous()
        if self.training:
            h = chain.train_forward(self, x, audio_lengths if self.mask_input else None)
        else:
            plan = self._plan(x.device)
            plan.bank = self._bank_for(x)
            if lang_bank is not None and lang_bank.device != x.device:
                lang_bank.to(x.device)                                         # new addresses: retire the graphs captured on the old ones
                self._param_epoch = getattr(self, "_param_epoch", 0) + 1
            plan.lang_bank = lang_bank
            h = plan.forward(x, audio_lengths if self.mask_input else None)
        cfg = self.original_encoder.config
        n_ad = int(cfg.num_adapter_layers) if getattr(cfg, "add_adapter", False) else 0
        return h.transpose(-1, -2), feat_extract_output_lengths(cfg.conv_kernel, cfg.conv_stride, audio_lengths, n_ad, int(getattr(cfg, "adapter_stride", 2)))
