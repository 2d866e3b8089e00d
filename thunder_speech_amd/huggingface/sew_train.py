"""SEW fine-tuning on the HIP kernels: the training-mode forward of `transformers.SEWModel` (models/sew/modeling_sew.py) as a chain of autograd nodes
whose forward and backward are C-ABI launches, in MIXED PRECISION only (`train_precision="bf16"`).  SEW's layers are wav2vec2's post-LN layers at
1 / squeeze_factor of the frame rate, so everything but the two ends of the encoder is huggingface/train.py's (post_ln_layer with LinearMixed, LayerNorm,
AttentionFused at head_dim 64 and FFNActLinear; BiasGelu, Dropout, mask_time, MaskRows, frozen_features); this module adds what is SEW's own, on
csrc/sew_train.hip (include/thunder_speech_amd/sew_train.h):

    SqueezeGelu       y[r] = mean_{i < s} x[s r + i] + gelu(conv_stride_s(x)[r] + b): the inference kernel with the conv result kept
                      (ts_sew_squeeze_train_fwd); backward: GELU backward, bias column sum, ts_sew_squeeze_dgrad (pool^T + conv^T on the matrix
                      cores, one launch), ts_sew_squeeze_wgrad
    UnsqueezeRows     the zero rows behind the upsampler when T % s != 0 (ts_sew_unsqueeze_rows); backward: the first s T2 rows of each clip
                      (ts_w2v_pad_rows)

transformers' training-mode forward, in order: frozen conv feature extractor; `layer_norm` over conv_dim[-1]; `feature_projection` (a plain Linear,
only when conv_dim[-1] != hidden_size); `feature_dropout`; time masking with `masked_spec_embed` -- SEWModel calls `_mask_hidden_states` WITHOUT the
attention mask, so the spans are drawn over all T frames and can fall on padded ones, unlike wav2vec2; padded rows zeroed at the full frame rate; the
squeeze; `encoder.layer_norm`, `dropout(hidden_dropout)`; the post-LN layers at T2 = T // s frames with min(ceil(len / s), T2) valid keys -- LayerDrop
drawn by torch.rand([]) per layer; upsample gelu(Linear(C -> s C)) read row-major as [B][s T2][C]; zero rows up to T.  The parameters stay the
transformers module's own; the conv's effective weight is built from (g, v) by torch ops on the parameters, so autograd carries d wk back through the
weight norm."""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from .. import _lib
from . import train as T
from .sew import SQUEEZE_SLOT, pooled_key_lengths, squeeze_on_matrix_cores
from .train import _f32c, _s

__all__ = ["train_forward", "refuse_untrainable", "squeeze_trains", "pack_squeeze_dgrad_taps", "SqueezeGelu", "UnsqueezeRows"]


def squeeze_trains(channels_per_group: int, kernel: int, stride: int) -> bool:
    """Whether the three launches of thunder_speech_amd/sew_train.h take this geometry (ts_sew_squeeze_train_supported): the geometries the inference call runs on
    its matrix-core kernel -- 24 or 32 channels per group, the staged window within 64 KiB of LDS.  Python mirror of the launchers' check."""
    return stride >= 1 and kernel >= 1 and squeeze_on_matrix_cores(channels_per_group, kernel, stride)


def pack_squeeze_dgrad_taps(wk: Tensor, stride: int) -> Tensor:
    """Effective conv weight as taps wk [k][g][out][in] -> the layout of ts_sew_squeeze_dgrad: bf16 [s][nt][g][32 in][32 out], nt = ceil(k / s); block
    (f, u) is the transposed tap j = f + s (nt - 1 - u), zeros where j >= k, zero-padded to 32 x 32."""
    k, g, cg, _ = wk.shape
    nt = -(-k // stride)
    out = torch.zeros(stride, nt, g, SQUEEZE_SLOT, SQUEEZE_SLOT, dtype=torch.bfloat16, device=wk.device)
    wt = wk.detach().transpose(2, 3).to(torch.bfloat16)
    for f in range(stride):
        js = [f + stride * (nt - 1 - u) for u in range(nt)]
        us = [u for u, j in enumerate(js) if j < k]
        if us:
            out[f, us, :, :cg, :cg] = wt[[js[u] for u in us]]
    return out


def refuse_untrainable(adapt) -> None:
    """Raise NotImplementedError, by name, for a SEW configuration the chain below has no backward for.  No device work: the adapter calls it before
    its GPU check."""
    T.refuse_untrainable_lora(adapt)                  # (lora_finetuning() refuses sew: only a hand-attached `lora` gets here)
    enc = adapt.original_encoder
    cfg = enc.config
    precision = getattr(adapt, "train_precision", "fp32")
    if precision != "bf16":
        raise NotImplementedError(f"sew: fine-tuning is not implemented with train_precision={precision!r} (the squeeze trains on the matrix-core "
                                  'kernels only); use train_precision="bf16", or the module in eval mode')
    if not T.FUSED_ATTENTION:
        raise NotImplementedError("sew: fine-tuning runs on the fused attention only (train.FUSED_ATTENTION is False)")
    c, g = int(cfg.hidden_size), int(cfg.num_conv_pos_embedding_groups)
    k, s = int(cfg.num_conv_pos_embeddings), int(cfg.squeeze_factor)
    if not squeeze_trains(c // g, k, s):
        raise NotImplementedError(f"sew fine-tuning: {c // g} channels per group with num_conv_pos_embeddings={k} and squeeze_factor={s} has no backward "
                                  "(24 or 32 channels per group train, with the staged window of 127 squeeze_factor + num_conv_pos_embeddings rows "
                                  "within 64 KiB of LDS); use the module in eval mode")
    T.refuse_masking_and_unfrozen(enc, "sew fine-tuning")


class SqueezeGelu(torch.autograd.Function):
    """y [B][T // s][C] = avg_pool(x, s) + gelu(grouped_conv1d(x, w, stride = s, padding = k // 2) + b) (SEWEncoder.forward: pool + pos_conv_embed).
    wk: the effective (weight-normalised) conv weight as [k][groups][out][in] f32 -- computed from (g, v) by torch ops on the PARAMETERS, as
    train.PosConvGelu's; x [B, T, C] time-major.  bf16 conv operands, f32 accumulation, pool, GELU and gradients.  Saved: x, the conv result z, wk, bias."""

    @staticmethod
    def forward(ctx, x, wk, bias, stride):
        x, wk, bias = _f32c(x), _f32c(wk), _f32c(bias)
        b, t, c = x.shape
        k, g, cg, _ = wk.shape
        t2 = t // stride
        L = _lib.lib()
        w16 = torch.zeros(k, g, SQUEEZE_SLOT, SQUEEZE_SLOT, dtype=torch.bfloat16, device=x.device)
        w16[:, :, :cg, :cg] = wk.to(torch.bfloat16)
        ws = torch.empty(L.ts_sew_squeeze_workspace_bytes(b, t, c, k, stride, 1), dtype=torch.uint8, device=x.device)
        y = torch.empty(b, t2, c, dtype=torch.float32, device=x.device)
        z = torch.empty_like(y)
        _lib.check(L.ts_sew_squeeze_train_fwd(x.data_ptr(), b, t, c, w16.data_ptr(), bias.data_ptr(), k, g, stride, y.data_ptr(), z.data_ptr(),
                                              ws.data_ptr(), _s(x)), "ts_sew_squeeze_train_fwd")
        ctx.save_for_backward(x, z, wk, bias)
        ctx.stride = stride
        return y

    @staticmethod
    def backward(ctx, dy):
        x, z, wk, bias = ctx.saved_tensors
        s = ctx.stride
        b, t, c = x.shape
        k, g, cg, _ = wk.shape
        dy = _f32c(dy)
        dev = dy.device
        L = _lib.lib()
        dz = torch.empty_like(dy)
        _lib.check(L.ts_w2v_gelu_bwd(z.data_ptr(), bias.data_ptr(), c, dy.data_ptr(), dz.data_ptr(), dz.numel(), _s(dy)), "ts_w2v_gelu_bwd")
        db = T._colsum(dz, dz.numel() // c, c) if ctx.needs_input_grad[2] else None
        dx = dwk = None
        if ctx.needs_input_grad[0]:
            wd16 = pack_squeeze_dgrad_taps(wk, s)
            ws = torch.empty(L.ts_sew_squeeze_dgrad_workspace_bytes(b, t, c, k, s), dtype=torch.uint8, device=dev)
            dx = torch.empty_like(x)
            _lib.check(L.ts_sew_squeeze_dgrad(dz.data_ptr(), dy.data_ptr(), b, t, c, wd16.data_ptr(), k, g, s, dx.data_ptr(), ws.data_ptr(), _s(dy)),
                       "ts_sew_squeeze_dgrad")
        if ctx.needs_input_grad[1]:
            dwk = torch.empty_like(wk)
            ws = torch.empty(L.ts_sew_squeeze_wgrad_workspace_bytes(b, t, c, k, s), dtype=torch.uint8, device=dev)
            _lib.check(L.ts_sew_squeeze_wgrad(dz.data_ptr(), x.data_ptr(), b, t, c, k, g, s, dwk.data_ptr(), ws.data_ptr(), _s(dy)), "ts_sew_squeeze_wgrad")
        return dx, dwk, db, None


class UnsqueezeRows(torch.autograd.Function):
    """up [B][T2][s C] (row-major [B][s T2][C]) -> [B][T][C] with zero rows s T2 .. T - 1 (SEWEncoder.forward's nn.functional.pad behind the upsampler);
    the backward keeps the first s T2 rows of each clip."""

    @staticmethod
    def forward(ctx, up, t, stride):
        up = _f32c(up)
        b, t2, sc = up.shape
        c = sc // stride
        out = torch.empty(b, t, c, dtype=torch.float32, device=up.device)
        _lib.check(_lib.lib().ts_sew_unsqueeze_rows(up.data_ptr(), b, t2, t, c, stride, out.data_ptr(), _s(up)), "ts_sew_unsqueeze_rows")
        ctx.geom = (b, t2, t, c, stride)
        return out

    @staticmethod
    def backward(ctx, dout):
        b, t2, t, c, stride = ctx.geom
        dout = _f32c(dout)
        dup = torch.empty(b, t2, stride * c, dtype=torch.float32, device=dout.device)
        _lib.check(_lib.lib().ts_w2v_pad_rows(dout.data_ptr(), dup.data_ptr(), b, stride * t2, t, 0, c, 1, _s(dout)), "ts_w2v_pad_rows")
        return dup, None, None


def train_forward(adapt, audio: Tensor, lengths: Optional[Tensor]) -> Tensor:
    """Training-mode SEWModel.forward -> last_hidden_state [B, T, C] (f32, time-major).  `adapt`: the HuggingFaceEncoderAdapt module (its
    `original_encoder` owns the parameters), with train_precision == "bf16"."""
    refuse_untrainable(adapt)
    with T.mixed_precision(True):                     # train.linear: LinearMixed; train.attention: AttentionFused
        return _train_forward(adapt, audio, lengths)


def _train_forward(adapt, audio: Tensor, lengths: Optional[Tensor]) -> Tensor:
    from .encoder import feat_extract_output_lengths
    enc = adapt.original_encoder
    cfg = enc.config
    dev = audio.device
    c, heads, s = int(cfg.hidden_size), int(cfg.num_attention_heads), int(cfg.squeeze_factor)
    if not T.AttentionFused.supported(c, heads):
        raise NotImplementedError(f"sew fine-tuning: head_dim={c // heads} (the fused attention takes 64)")
    feats = T.frozen_features(adapt, audio)
    b, t, _ = feats.shape
    if t < s:
        raise RuntimeError(f"sew: input too short: {t} frames behind the conv feature extractor, squeeze_factor {s}")
    t2 = t // s
    eps = float(cfg.layer_norm_eps)
    en = enc.encoder
    h = T.LayerNorm.apply(feats, None, enc.layer_norm.weight, enc.layer_norm.bias, eps)
    if getattr(enc, "project_features", int(cfg.conv_dim[-1]) != c):
        h = T.linear(h, enc.feature_projection.weight, enc.feature_projection.bias)
    h = T.dropout(h, float(cfg.feat_proj_dropout))
    h = T.mask_time(enc, h, None)                           # SEWModel._mask_hidden_states gets no attention mask: spans over all t frames of every clip
    key_len = None
    if lengths is not None:
        frames = feat_extract_output_lengths(cfg.conv_kernel, cfg.conv_stride, lengths.to(dev).long())
        key_len = pooled_key_lengths(frames, s, t2).to(torch.int32).contiguous()
        h = T.MaskRows.apply(h, frames.to(torch.int32).contiguous())
    # squeeze: the weight norm on the parameters, pool + conv + GELU on the kernels
    conv = en.pos_conv_embed.conv
    h = SqueezeGelu.apply(h, T.weight_normed_taps(conv, int(cfg.num_conv_pos_embedding_groups)), conv.bias, s)
    h = T.LayerNorm.apply(h, None, en.layer_norm.weight, en.layer_norm.bias, eps)
    p_hid, p_act, p_att = float(cfg.hidden_dropout), float(cfg.activation_dropout), float(cfg.attention_dropout)
    h = T.dropout(h, p_hid)
    for layer in en.layers:
        if torch.rand([]).item() < float(cfg.layerdrop):       # LayerDrop, drawn as transformers draws it
            continue
        att = layer.attention
        wqkv, bqkv = T.stacked_qkv(att)
        # (mixed mode, FUSED_ATTENTION and head_dim 64, all checked above: train.attention takes AttentionFused)
        h = T.post_ln_layer(layer, h, lambda x: T.self_attention(att, x, wqkv, bqkv, key_len, heads, p_att, p_hid), p_act, p_hid, eps)
    up = en.upsample.projection
    u = T.BiasGelu.apply(T.linear(h, up.weight, None), up.bias)            # [B][T2][s C] = [B][s T2][C] row-major
    if s * t2 == t:
        return u.view(b, t, c)
    return UnsqueezeRows.apply(u, t, s)
