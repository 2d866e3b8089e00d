"""wav2vec2-conformer (rotary) fine-tuning on the HIP kernels: the training-mode forward of `transformers.Wav2Vec2ConformerModel` as a chain of
autograd nodes whose forward and backward are C-ABI launches, in MIXED PRECISION only (`train_precision="bf16"`).  Everything a conformer layer
shares with wav2vec2 is huggingface/train.py's (LinearMixed, AttentionFused, FFNActLinear, LayerNorm, Dropout, mask_time, MaskRows, Add,
frozen_features); this module adds what is the conformer's own, on csrc/conformer_train.hip (include/thunder_speech_amd/conformer_train.h):

    LayerNormRotary    LN(h) and its rotated copy (the inference launch ts_conformer_layernorm_rotary_fwd at f32); backward: ts_conformer_rotary_bwd,
                       then the LayerNorm backward
    RotaryQKV          q | k = linear(rot(LN h), cat(Wq, Wk)), v = linear(LN h, Wv) into the column slices of ONE [B][t][3c] buffer -- the GEMM takes
                       the output pitch and the cast launch the input pitch, so nothing is concatenated or sliced by a launch of its own
    GluDwconvBnAct     pointwise_conv2(act(BatchNorm(depthwise_conv(GLU(u))))): three forward launches (conv + statistics partials, statistics,
                       BatchNorm + activation straight to the bf16 operands) and, backward, the data-gradient product, the d gamma / d beta sums and
                       ONE launch for BatchNorm, transposed conv, weight gradient and GLU

transformers' training-mode forward (modeling_wav2vec2_conformer.py): frozen conv feature extractor, feature projection with its dropout, time
masking, padded rows zeroed, `hidden_dropout`, NO positional conv (Wav2Vec2ConformerEncoder builds it and never calls it: its parameters get no
gradient on either side), then per layer -- LayerDrop drawn by torch.rand([]) --

    h += 0.5 ffn1(LN(h));   h += drop(attn(LN(h)));   h += drop_conv(conv_module(h));   h += 0.5 ffn2(LN(h));   h = LN(h)

and `encoder.layer_norm`.  The 0.5 is folded into output_dense by torch ops on the PARAMETERS (0.5 W, 0.5 b: exact, autograd carries it back; dropout
commutes with the scale).  BatchNorm follows the module: in training it normalises with the statistics of all B t frames of the padded batch and
updates running_mean / running_var / num_batches_tracked (torch ops on [c] tensors, under no_grad); a batch_norm put in eval() inside a training
encoder uses its running statistics forward and backward and updates nothing.  The five LayerNorms of a layer use eps 1e-5, the projection's and the
encoder's config.layer_norm_eps.  Under parallel.py's data parallelism every rank keeps its own running statistics (no SyncBatchNorm), as torch DDP does."""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from .. import _lib
from ..rng import next_seed
from . import train as T
from .conformer import CONFORMER_ACTS, INNER_EPS, rotary_table
from .train import _f32c, _pad32, _s

__all__ = ["train_forward", "refuse_untrainable", "LayerNormRotary", "RotaryQKV", "GluDwconvBnAct"]


def refuse_untrainable(adapt) -> None:
    """Raise NotImplementedError, by name, for a wav2vec2-conformer configuration the chain below has no backward for.  No device work: the adapter
    calls it before its GPU check."""
    T.refuse_untrainable_lora(adapt)                  # (lora_finetuning() refuses the conformer: only a hand-attached `lora` gets here)
    enc = adapt.original_encoder
    cfg = enc.config
    precision = getattr(adapt, "train_precision", "fp32")
    if precision != "bf16":
        raise NotImplementedError(f"wav2vec2-conformer: fine-tuning with train_precision={precision!r} is not implemented (the conformer chain "
                                  'trains in mixed precision only); use train_precision="bf16", or the module in eval mode')
    if not T.FUSED_ATTENTION:
        raise NotImplementedError("wav2vec2-conformer: fine-tuning runs on the fused attention only (train.FUSED_ATTENTION is False)")
    if getattr(cfg, "add_adapter", False):
        raise NotImplementedError("wav2vec2-conformer fine-tuning: add_adapter=True is inference-only (the adapter layers have no backward here)")
    T.refuse_masking_and_unfrozen(enc, "wav2vec2-conformer fine-tuning")
    if int(cfg.intermediate_size) % 32:
        raise NotImplementedError(f"wav2vec2-conformer fine-tuning: intermediate_size={cfg.intermediate_size} (the fused feed-forward activation "
                                  "takes multiples of 32)")


def _gemm_nt_pitch(a16: Tensor, lda: int, w16: Tensor, ldw: int, out_ptr: int, ldc: int, rows: int, n: int, k: int, bias: Optional[Tensor], stream) -> None:
    """train._gemm_nt into a column slice: out[r][j] (f32, row pitch ldc, at address out_ptr) = sum_i a16[r][i] w16[j][i] + bias[j]."""
    st = _lib.lib().ts_gemm_nt_bf16(a16.data_ptr(), lda, w16.data_ptr(), ldw, bias.data_ptr() if bias is not None else None, None, 0, out_ptr, ldc,
                                    None, 0, rows, n, k, 0, stream)
    _lib.check(st, "ts_gemm_nt_bf16")


def _cast_pitch(x_ptr: int, ldx: int, rows: int, c: int, dev, colsum: Tensor):
    """train._cast of a column slice: (bf16 [rows][c], bf16 [c][pad32(rows)]) of the f32 columns at x_ptr (row pitch ldx); their sums are added to colsum."""
    rp = _pad32(rows)
    y = torch.empty(rows, c, dtype=torch.bfloat16, device=dev)
    yt = torch.empty(c, rp, dtype=torch.bfloat16, device=dev)
    st = _lib.lib().ts_w2v_cast_bf16_t_colsum(x_ptr, ldx, rows, c, y.data_ptr(), c, yt.data_ptr(), rp, rp, colsum.data_ptr(),
                                              torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(st, "ts_w2v_cast_bf16_t_colsum")
    return y, yt


class LayerNormRotary(torch.autograd.Function):
    """(y, y_rot) = (LN(x), rot(LN(x))) over heads of 64 channels, positions = frames of the padded batch (Wav2Vec2ConformerSelfAttention.
    _apply_rotary_embedding on the output of self_attn_layer_norm).  cos_sin: conformer.rotary_table on the device, [2][t_table][32]."""

    @staticmethod
    def forward(ctx, x, gamma, beta, cos_sin, t_table, heads):
        x = _f32c(x)
        b, t, c = x.shape
        y, yr = torch.empty_like(x), torch.empty_like(x)
        st = _lib.lib().ts_conformer_layernorm_rotary_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), INNER_EPS, b, t, c, heads, cos_sin.data_ptr(),
                                                          t_table, 0, y.data_ptr(), yr.data_ptr(), _s(x))
        _lib.check(st, "ts_conformer_layernorm_rotary_fwd")
        ctx.save_for_backward(x, gamma, cos_sin)
        ctx.t_table = t_table
        return y, yr

    @staticmethod
    def backward(ctx, dy_v, dy_r):
        x, gamma, cos_sin = ctx.saved_tensors
        dy_v, dy_r = _f32c(dy_v), _f32c(dy_r)
        b, t, c = x.shape
        rows = b * t
        L = _lib.lib()
        dy = torch.empty_like(x)
        _lib.check(L.ts_conformer_rotary_bwd(dy_v.data_ptr(), dy_r.data_ptr(), b, t, c, cos_sin.data_ptr(), ctx.t_table, dy.data_ptr(), _s(x)),
                   "ts_conformer_rotary_bwd")
        dx = torch.empty_like(x)
        dg = torch.empty(c, dtype=torch.float32, device=x.device)
        db = torch.empty(c, dtype=torch.float32, device=x.device)
        ws = torch.empty(L.ts_w2v_layernorm_bwd_workspace(rows, c), dtype=torch.uint8, device=x.device)
        st = L.ts_w2v_layernorm_bwd_set(x.data_ptr(), None, gamma.data_ptr(), dy.data_ptr(), INNER_EPS, rows, c, dx.data_ptr(), dg.data_ptr(), db.data_ptr(),
                                        ws.data_ptr(), _s(x))
        _lib.check(st, "ts_w2v_layernorm_bwd_set")
        return dx, dg, db, None, None, None


class RotaryQKV(torch.autograd.Function):
    """qkv [B][t][3c] f32: columns [0, 2c) = y_rot cat(Wq, Wk)^T + cat(bq, bk), columns [2c, 3c) = y Wv^T + bv -- LinearMixed's three products per
    branch (bf16 operands, f32 accumulation, split-K weight gradients), the bias gradients out of the launches that cast the two slices of d qkv."""

    @staticmethod
    def forward(ctx, y, yr, wqk, bqk, wv, bv):
        y, yr, wqk, wv = _f32c(y), _f32c(yr), _f32c(wqk), _f32c(wv)
        b, t, c = y.shape
        rows = b * t
        need_w = ctx.needs_input_grad[2] or ctx.needs_input_grad[4]
        yr16, yrt16 = T._cast(yr.view(rows, c), rows, c, True, need_w)
        y16, yt16 = T._cast(y.view(rows, c), rows, c, True, need_w)
        wqk16, wqkt16 = T._cast(wqk, 2 * c, c, True, True)
        wv16, wvt16 = T._cast(wv, c, c, True, True)
        qkv = torch.empty(b, t, 3 * c, dtype=torch.float32, device=y.device)
        _gemm_nt_pitch(yr16, c, wqk16, c, qkv.data_ptr(), 3 * c, rows, 2 * c, c, _f32c(bqk), _s(y))
        _gemm_nt_pitch(y16, c, wv16, c, qkv.data_ptr() + 8 * c, 3 * c, rows, c, c, _f32c(bv), _s(y))
        ctx.save_for_backward(yrt16, yt16, wqkt16, wvt16)
        ctx.geom = (b, t, c)
        return qkv

    @staticmethod
    def backward(ctx, dqkv):
        yrt16, yt16, wqkt16, wvt16 = ctx.saved_tensors
        b, t, c = ctx.geom
        rows, rp = b * t, _pad32(b * t)
        dqkv = _f32c(dqkv)
        dev = dqkv.device
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        dbqk, dbv = torch.zeros(2 * c, dtype=torch.float32, device=dev), torch.zeros(c, dtype=torch.float32, device=dev)
        dqk16, dqkt16 = _cast_pitch(dqkv.data_ptr(), 3 * c, rows, 2 * c, dev, dbqk)
        dv16, dvt16 = _cast_pitch(dqkv.data_ptr() + 8 * c, 3 * c, rows, c, dev, dbv)
        dy = dyr = dwqk = dwv = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            dyr, dy = new(b, t, c), new(b, t, c)
            T._gemm_nt_splitk(dqk16, 2 * c, wqkt16, _pad32(2 * c), dyr, rows, c, 2 * c)
            T._gemm_nt_splitk(dv16, c, wvt16, _pad32(c), dy, rows, c, c)
        if yrt16 is not None:
            dwqk, dwv = new(2 * c, c), new(c, c)
            T._gemm_nt_splitk(dqkt16, rp, yrt16, rp, dwqk, 2 * c, c, rp)
            T._gemm_nt_splitk(dvt16, rp, yt16, rp, dwv, c, c, rp)
        return dy, dyr, dwqk, dbqk, dwv, dbv


class GluDwconvBnAct(torch.autograd.Function):
    """(pointwise_conv2(act(BatchNorm(depthwise_conv(GLU(u))))), (mean, biased variance) of the batch) of Wav2Vec2ConformerConvolutionModule, from
    u = pointwise_conv1(LN(h)) [B][t][2c] f32.  dw [k][c]: the depthwise weight tap-major (a permuted copy made by torch ops on the parameter, so
    autograd carries its gradient back); w2 [c][c].  `running`: None for batch statistics, else f32 [2][c] = (running_mean, 1 / sqrt(running_var +
    eps)) -- BatchNorm in eval mode.  Saved for the backward: u, z, the statistics and the transposed bf16 operands of the product; the activation
    exists as bf16 operands only, dz never exists in memory."""

    @staticmethod
    def forward(ctx, u, dw, gamma, beta, w2, running, act, eps):
        u, dw, gamma, beta, w2 = _f32c(u), _f32c(dw), _f32c(gamma), _f32c(beta), _f32c(w2)
        b, t, c2 = u.shape
        c, k = c2 // 2, dw.shape[0]
        rows, rp = b * t, _pad32(b * t)
        dev = u.device
        L = _lib.lib()
        z = torch.empty(b, t, c, dtype=torch.float32, device=dev)
        ws = torch.empty(L.ts_conformer_glu_dwconv_train_fwd_workspace(b, t, c), dtype=torch.uint8, device=dev)
        _lib.check(L.ts_conformer_glu_dwconv_train_fwd(u.data_ptr(), b, t, c, dw.data_ptr(), k, z.data_ptr(), ws.data_ptr(), _s(u)),
                   "ts_conformer_glu_dwconv_train_fwd")
        if running is None:
            mean_rstd = torch.empty(2, c, dtype=torch.float32, device=dev)
            mean_var = torch.empty(2, c, dtype=torch.float32, device=dev)
            _lib.check(L.ts_conformer_bn_stats(ws.data_ptr(), b, t, c, float(eps), mean_rstd.data_ptr(), mean_var.data_ptr(), _s(u)), "ts_conformer_bn_stats")
        else:
            mean_rstd, mean_var = _f32c(running), torch.empty(0, dtype=torch.float32, device=dev)
        a16 = torch.empty(rows, c, dtype=torch.bfloat16, device=dev)
        at16 = torch.empty(c, rp, dtype=torch.bfloat16, device=dev) if ctx.needs_input_grad[4] else None
        _lib.check(L.ts_conformer_bn_act_cast(z.data_ptr(), mean_rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), rows, c, int(act), a16.data_ptr(),
                                              at16.data_ptr() if at16 is not None else None, rp, rp, _s(u)), "ts_conformer_bn_act_cast")
        w16, wt16 = T._cast(w2, c, c, True, True)
        y = torch.empty(b, t, c, dtype=torch.float32, device=dev)
        T._gemm_nt_splitk(a16, c, w16, c, y, rows, c, c, min_k=2048)
        ctx.save_for_backward(u, z, mean_rstd, gamma, beta, dw, at16, wt16)
        ctx.geom = (b, t, c, k, int(act), running is not None)
        ctx.mark_non_differentiable(mean_var)
        return y, mean_var

    @staticmethod
    def backward(ctx, dy, _):
        u, z, mean_rstd, gamma, beta, dw, at16, wt16 = ctx.saved_tensors
        b, t, c, k, act, running = ctx.geom
        rows, rp = b * t, _pad32(b * t)
        dy = _f32c(dy)
        dev = dy.device
        L = _lib.lib()
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        dy16, dyt16 = T._cast(dy.view(rows, c), rows, c, True, at16 is not None)
        da = new(rows, c)
        T._gemm_nt_splitk(dy16, c, wt16, _pad32(c), da, rows, c, c)
        dw2 = None
        if at16 is not None:
            dw2 = new(c, c)
            T._gemm_nt_splitk(dyt16, rp, at16, rp, dw2, c, c, rp)
        dgamma, dbeta = new(c), new(c)
        ws = torch.empty(L.ts_conformer_bn_act_bwd_sums_workspace(rows, c), dtype=torch.uint8, device=dev)
        _lib.check(L.ts_conformer_bn_act_bwd_sums(z.data_ptr(), mean_rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), da.data_ptr(), rows, c, act,
                                                  dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(), _s(dy)), "ts_conformer_bn_act_bwd_sums")
        du, ddw = torch.empty_like(u), new(k, c)
        ws = torch.empty(L.ts_conformer_glu_dwconv_train_bwd_workspace(b, t, c, k), dtype=torch.uint8, device=dev)
        _lib.check(L.ts_conformer_glu_dwconv_train_bwd(u.data_ptr(), z.data_ptr(), da.data_ptr(), b, t, c, dw.data_ptr(), k, mean_rstd.data_ptr(),
                                                       gamma.data_ptr(), beta.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), int(running), act,
                                                       du.data_ptr(), ddw.data_ptr(), ws.data_ptr(), _s(dy)), "ts_conformer_glu_dwconv_train_bwd")
        return du, ddw, dgamma, dbeta, dw2, None, None, None


def _rotary(adapt, en, t: int, dev):
    """(device rotary table [2][t_table][32], t_table) for t frames, kept on the adapter and grown when a batch is longer."""
    kept = adapt.__dict__.setdefault("_train_rotary", {})
    hit = kept.get(str(dev))
    if hit is None or hit[1] < t:
        t_table = max(t, int(getattr(en.config, "max_source_positions", 5000)))
        hit = (rotary_table(en.embed_positions.inv_freq, t_table).to(dev), t_table)
        kept[str(dev)] = hit
    return hit


def train_forward(adapt, audio: Tensor, lengths: Optional[Tensor]) -> Tensor:
    """Training-mode Wav2Vec2ConformerModel.forward -> last_hidden_state [B, T', C] (f32, time-major).  `adapt`: the HuggingFaceEncoderAdapt module
    (its `original_encoder` owns the parameters), with train_precision == "bf16"."""
    refuse_untrainable(adapt)
    with T.mixed_precision(True):                     # train.linear / train.attention: LinearMixed and the fused attention
        return _train_forward(adapt, audio, lengths)


def _train_forward(adapt, audio: Tensor, lengths: Optional[Tensor]) -> Tensor:
    from .encoder import feat_extract_output_lengths
    enc = adapt.original_encoder
    cfg = enc.config
    dev = audio.device
    c, heads = int(cfg.hidden_size), int(cfg.num_attention_heads)
    frames = int(feat_extract_output_lengths(cfg.conv_kernel, cfg.conv_stride, torch.tensor([audio.shape[1]])))
    if audio.shape[0] * frames < 2 and any(layer.conv_module.batch_norm.training for layer in enc.encoder.layers):
        # one frame in the whole batch: BatchNorm has no variance to normalise with; torch's own check and message, before any launch
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {torch.Size([audio.shape[0], c, frames])}")
    feats = T.frozen_features(adapt, audio)
    b, t, _ = feats.shape
    eps = float(cfg.layer_norm_eps)
    fp, en = enc.feature_projection, enc.encoder
    h = T.LayerNorm.apply(feats, None, fp.layer_norm.weight, fp.layer_norm.bias, eps)
    h = T.linear(h, fp.projection.weight, fp.projection.bias)
    h = T.dropout(h, float(cfg.feat_proj_dropout))
    key_len = None
    if lengths is not None:
        key_len = feat_extract_output_lengths(cfg.conv_kernel, cfg.conv_stride, lengths.to(dev).long()).to(torch.int32).contiguous()
    h = T.mask_time(enc, h, key_len)
    if key_len is not None:
        h = T.MaskRows.apply(h, key_len)
    p_hid, p_act, p_att = float(cfg.hidden_dropout), float(cfg.activation_dropout), float(cfg.attention_dropout)
    p_conv = float(cfg.conformer_conv_dropout)
    h = T.dropout(h, p_hid)
    cos_sin, t_table = _rotary(adapt, en, t, dev)
    act = CONFORMER_ACTS[cfg.hidden_act]
    k = int(cfg.conv_depthwise_kernel_size)
    if not T.AttentionFused.supported(c, heads):
        raise NotImplementedError(f"wav2vec2-conformer fine-tuning: head_dim={c // heads} (the fused attention and the rotary kernels take 64)")

    def ln(x, norm, res=None):
        return T.LayerNorm.apply(x, res, norm.weight, norm.bias, INNER_EPS)

    def ffn(ff, x):
        z = T.linear(x, ff.intermediate_dense.weight, None)
        y = T.FFNActLinear.apply(z, ff.intermediate_dense.bias, 0.5 * ff.output_dense.weight, 0.5 * ff.output_dense.bias, p_act,
                                 next_seed() if p_act > 0 else 0, act)
        return T.dropout(y, p_hid)

    def conv_module(m, x):
        u = T.linear(ln(x, m.layer_norm), m.pointwise_conv1.weight.squeeze(-1), None)
        bn = m.batch_norm
        batch_stats = bn.training or bn.running_mean is None
        running = None
        if not batch_stats:
            with torch.no_grad():
                running = torch.stack([bn.running_mean.float(), torch.rsqrt(bn.running_var.float() + bn.eps)]).contiguous()
        y, mean_var = GluDwconvBnAct.apply(u, m.depthwise_conv.weight.view(c, k).t().contiguous(), bn.weight, bn.bias,
                                           m.pointwise_conv2.weight.squeeze(-1), running, act, float(bn.eps))
        if bn.training and bn.track_running_stats and bn.running_mean is not None:
            with torch.no_grad():
                n = b * t
                bn.num_batches_tracked += 1
                mom = float(bn.momentum) if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)
                bn.running_mean.mul_(1.0 - mom).add_(mean_var[0], alpha=mom)
                bn.running_var.mul_(1.0 - mom).add_(mean_var[1], alpha=mom * n / (n - 1))
        return T.dropout(y, p_conv)

    for layer in en.layers:
        if torch.rand([]).item() < float(cfg.layerdrop):       # LayerDrop, drawn as transformers draws it
            continue
        att = layer.self_attn
        h = T.Add.apply(h, ffn(layer.ffn1, ln(h, layer.ffn1_layer_norm)))
        y, yr = LayerNormRotary.apply(h, layer.self_attn_layer_norm.weight, layer.self_attn_layer_norm.bias, cos_sin, t_table, heads)
        qkv = RotaryQKV.apply(y, yr, torch.cat([att.linear_q.weight, att.linear_k.weight], 0), torch.cat([att.linear_q.bias, att.linear_k.bias], 0),
                              att.linear_v.weight, att.linear_v.bias)
        ctxt = T.attention(qkv, key_len, heads, p_att, next_seed() if p_att > 0 else 0)
        # (Wav2Vec2ConformerEncoderLayer.self_attn_dropout is built with attention_dropout, not hidden_dropout)
        h = T.Add.apply(h, T.dropout(T.linear(ctxt, att.linear_out.weight, att.linear_out.bias), p_att))
        h = T.Add.apply(h, conv_module(layer.conv_module, h))
        h = ln(ffn(layer.ffn2, ln(h, layer.ffn2_layer_norm)), layer.final_layer_norm, res=h)      # LN(h + 0.5 ffn2(..)): the add rides in the launch
    return T.LayerNorm.apply(h, None, en.layer_norm.weight, en.layer_norm.bias, eps)
