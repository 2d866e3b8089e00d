"""wav2vec2-conformer encoder (rotary position embeddings) on the HIP kernels of csrc/conformer.hip and the wav2vec2 files (csrc/w2v_conv.hip, w2v_rows.hip, w2v_posconv.hip, w2v_attn.hip).

transformers modeling_wav2vec2_conformer.py, reached from the reference's `_HuggingFaceEncoderAdapt.forward` (huggingface/compatibility.py:31-42)
for a wav2vec2-conformer checkpoint.  The feature extractor, the feature projection and the adapter are wav2vec2's (`Wav2Vec2Plan`); the encoder
is different: no positional conv (Wav2Vec2ConformerEncoder builds it but never calls it) and no LayerNorm in front of the layers, then per layer
(h: the f32 residual stream)

    h += 0.5 ffn1(LN(h));   h += attn(LN(h));   h += conv_module(h);   h += 0.5 ffn2(LN(h));   h = LN(h)

and `encoder.layer_norm` after the last one.  The five LayerNorms of a layer and the BatchNorm use eps 1e-5 whatever config.layer_norm_eps says;
the feature projection's and the encoder's LayerNorm use config.layer_norm_eps.  The attention multiplies rot(LN(h)) by linear_q and linear_k
and LN(h) by linear_v (rotary per head of 64, positions = frames of the padded batch), its core is the plain softmax attention of
ts_w2v_attention_fwd.  Padded frames are not masked after the encoder's input: the depthwise conv carries them into a shorter clip's last
frames, and the HIP path computes them exactly as transformers does."""
from __future__ import annotations

from typing import Dict, Optional

import torch

from .. import _lib
from .encoder import Wav2Vec2Plan, feat_extract_output_lengths

__all__ = ["ConformerPlan", "rotary_table", "CONFORMER_ACTS"]

# config.hidden_act -> the act code of the conformer launches (1: erf GELU, 2: SiLU)
CONFORMER_ACTS = {"gelu": 1, "swish": 2, "silu": 2}
INNER_EPS = 1e-5          # nn.LayerNorm / nn.BatchNorm1d defaults of the five LayerNorms and the BatchNorm inside a layer


def rotary_table(inv_freq: torch.Tensor, t: int) -> torch.Tensor:
    """float32 [2][t][32]: cos and sin of p inv_freq for frames p < t, with the float32 torch operations of
    Wav2Vec2ConformerRotaryPositionalEmbedding.forward (which repeats the 32 columns: cat((freqs, freqs), -1)); built on the host."""
    inv_freq = inv_freq.detach().to("cpu")
    time_stamps = torch.arange(t).type_as(inv_freq)
    freqs = torch.einsum("i,j->ij", time_stamps, inv_freq)
    embeddings = torch.cat((freqs, freqs), dim=-1)
    half = inv_freq.shape[0]
    return torch.stack([embeddings.cos()[:, :half], embeddings.sin()[:, :half]]).to(torch.float32).contiguous()


class ConformerPlan(Wav2Vec2Plan):
    """Packed weights + launch sequence of a Wav2Vec2ConformerModel (rotary).  precision as Wav2Vec2Plan: "fp32" or "bf16" (bf16 GEMM operands,
    f32 accumulation, residual stream, normalisations, softmax and depthwise conv)."""

    def __init__(self, cfg, sd: Dict[str, torch.Tensor], device, precision: str = "bf16"):
        # the base packs the conv feature extractor only: its full packing reads wav2vec2's layer keys and the unused positional conv
        super().__init__(cfg, sd, device, precision, feature_extractor_only=True)
        self.feature_extractor_only = False
        f = lambda k: sd[k].detach().to(device=self.device, dtype=torch.float32).contiguous()
        gw = (lambda t: t.to(torch.bfloat16).contiguous()) if self.prec else (lambda t: t.contiguous())
        self.act = CONFORMER_ACTS[cfg.hidden_act]
        self.kdw = int(cfg.conv_depthwise_kernel_size)
        # the feature projection (Wav2Vec2ConformerFeatureProjection always has its LayerNorm) and the adapter (Wav2Vec2ConformerAdapter is
        # Wav2Vec2Adapter: the base's _adapter runs it) are packed by the base's own helpers
        self._pack_projection(f, gw)
        self.enc_ln = (f("encoder.layer_norm.weight"), f("encoder.layer_norm.bias"))
        self._pack_adapter(cfg, sd, f)
        c = self.hidden
        for i in range(self.n_layers):
            q = f"encoder.layers.{i}."
            ln = lambda n: (f(q + n + ".weight"), f(q + n + ".bias"))
            lw = dict(ln_ffn1=ln("ffn1_layer_norm"), ln_attn=ln("self_attn_layer_norm"), ln_conv=ln("conv_module.layer_norm"),
                      ln_ffn2=ln("ffn2_layer_norm"), ln_final=ln("final_layer_norm"))
            for n in ("ffn1", "ffn2"):
                # the half step folded into output_dense: 0.5 W, 0.5 b (exact in f32 and bf16)
                lw[n] = (gw(f(q + n + ".intermediate_dense.weight")), f(q + n + ".intermediate_dense.bias"),
                         gw(0.5 * f(q + n + ".output_dense.weight")), (0.5 * f(q + n + ".output_dense.bias")).contiguous())
            a = q + "self_attn."
            lw.update(wqk=gw(torch.cat([f(a + "linear_q.weight"), f(a + "linear_k.weight")], 0)),
                      bqk=torch.cat([f(a + "linear_q.bias"), f(a + "linear_k.bias")], 0).contiguous(),
                      wv=gw(f(a + "linear_v.weight")), bv=f(a + "linear_v.bias"),
                      wo=gw(f(a + "linear_out.weight")), bo=f(a + "linear_out.bias"))
            m = q + "conv_module."
            bn = m + "batch_norm."
            scale = f(bn + "weight") / torch.sqrt(f(bn + "running_var") + INNER_EPS)
            lw.update(pw1=gw(f(m + "pointwise_conv1.weight").reshape(2 * c, c)), pw2=gw(f(m + "pointwise_conv2.weight").reshape(c, c)),
                      dw=f(m + "depthwise_conv.weight").reshape(c, self.kdw).t().contiguous(),          # [k][c]
                      bn_scale=scale.contiguous(), bn_shift=(f(bn + "bias") - f(bn + "running_mean") * scale).contiguous())
            self.layers.append(lw)
        self.inv_freq = sd["encoder.embed_positions.inv_freq"].detach().to("cpu", torch.float32)
        self._grow_rotary(int(getattr(cfg, "max_source_positions", 5000)))

    def _grow_rotary(self, t: int) -> None:
        """(Re)build the device rotary table for `t` frames.  A superseded table stays referenced for the plan's lifetime: graphs captured
        before the growth hold its address and its t_table as launch arguments, and replay them after it (a freed block would be handed to
        the next allocation and read as cos / sin with no error)."""
        if hasattr(self, "cos_sin"):
            self.__dict__.setdefault("_retired_tables", []).append(self.cos_sin)
        self.t_table = int(t)
        self.cos_sin = rotary_table(self.inv_freq, self.t_table).to(self.device)

    def _clinear(self, L, stream, x_op, w, bias, act=0, y_op=None, ld_op=0, res=None, want_op=False):
        """ts_conformer_linear_fwd: (f32 result or None, operand).  y_op: a bf16 (bf16 mode) or f32 (fp32 mode) column slice of a wider buffer
        with row pitch ld_op that receives the result; else want_op: a dense operand copy for the next product."""
        b, t, k = x_op.shape
        n = w.shape[0]
        rows = b * t
        if y_op is not None and not self.prec:                    # f32: the slice is the f32 result itself
            _lib.check(L.ts_conformer_linear_fwd(x_op.data_ptr(), x_op.stride(1), w.data_ptr(), None, self._ptr(bias), None, 0, y_op.data_ptr(), ld_op,
                                                 None, 0, rows, n, k, act, 0, stream), "ts_conformer_linear_fwd")
            return None, y_op
        if y_op is None and want_op and self.prec:
            y_op, ld_op = self._op(b, t, n), n
        y = None if (y_op is not None and res is None) else (res if res is not None else self._buf(b, t, n))
        _lib.check(L.ts_conformer_linear_fwd(x_op.data_ptr(), x_op.stride(1), w.data_ptr(), self._ptr(self._frag(w)), self._ptr(bias), self._ptr(res),
                                             n if res is not None else 0, self._ptr(y), n if y is not None else 0, self._ptr(y_op), ld_op, rows, n, k,
                                             act, self.prec, stream), "ts_conformer_linear_fwd")
        return y, (y_op if self.prec else y)

    def forward(self, audio: torch.Tensor, lengths: Optional[torch.Tensor]) -> torch.Tensor:
        """audio [B, n] fp32 on the GPU; lengths = samples per clip with `mask_input`, else None.  -> last_hidden_state [B, T', C] fp32."""
        L = _lib.lib()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        feats, _ = self._feature_extractor(audio)
        b, t, _ = feats.shape
        c = self.hidden
        if t > self.t_table:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"wav2vec2-conformer: {t} frames exceed the rotary table's {self.t_table} (config.max_source_positions) inside a "
                                   "graph capture; run the longest input once eagerly first, or raise max_source_positions")
            self._grow_rotary(t)
        _, ln_op = self._ln(L, stream, feats, self.fp_ln, want_f32=False)
        h, _ = self._linear(L, stream, ln_op, self.fp_w, self.fp_b)
        key_len = None
        if lengths is not None:
            key_len = feat_extract_output_lengths(self.kernels, self.strides, lengths.to(self.device).long()).to(torch.int32).contiguous()
            _lib.check(L.ts_w2v_mask_rows(h.data_ptr(), b, t, c, key_len.data_ptr(), stream), "ts_w2v_mask_rows")
        att_ws = self._buf(L.ts_w2v_attention_workspace_bytes(b, t, self.heads, self.prec), dtype=torch.uint8)
        op_dtype = torch.bfloat16 if self.prec else torch.float32

        def ffn(wts, ln):
            w1, b1, w2, b2 = wts
            _, x_op = self._ln(L, stream, h, ln, eps=INNER_EPS, want_f32=False)
            _, f_op = self._clinear(L, stream, x_op, w1, b1, act=self.act, want_op=True)
            self._linear(L, stream, f_op, w2, b2, into=h)                          # h += 0.5 output_dense(...): the half folded into w2, b2

        for lw in self.layers:
            ffn(lw["ffn1"], lw["ln_ffn1"])
            # attention: q | k from the rotated LayerNorm output, v from the plain one, into the column slices of one qkv buffer
            y_op, yr_op = self._buf(b, t, c, dtype=op_dtype), self._buf(b, t, c, dtype=op_dtype)
            _lib.check(L.ts_conformer_layernorm_rotary_fwd(h.data_ptr(), lw["ln_attn"][0].data_ptr(), lw["ln_attn"][1].data_ptr(), INNER_EPS, b, t, c,
                                                           self.heads, self.cos_sin.data_ptr(), self.t_table, self.prec, y_op.data_ptr(),
                                                           yr_op.data_ptr(), stream), "ts_conformer_layernorm_rotary_fwd")
            qkv = self._buf(b, t, 3 * c, dtype=op_dtype)
            self._clinear(L, stream, yr_op, lw["wqk"], lw["bqk"], y_op=qkv[:, :, :2 * c], ld_op=3 * c)
            self._clinear(L, stream, y_op, lw["wv"], lw["bv"], y_op=qkv[:, :, 2 * c:], ld_op=3 * c)
            ctx = self._buf(b, t, c, dtype=op_dtype)
            _lib.check(L.ts_w2v_attention_fwd(qkv.data_ptr(), b, t, c, self.heads, self._ptr(key_len), self.prec, ctx.data_ptr(), att_ws.data_ptr(),
                                              stream), "ts_w2v_attention_fwd")
            self._linear(L, stream, ctx, lw["wo"], lw["bo"], into=h)
            # convolution module: pw1 -> GLU -> depthwise -> BatchNorm -> act (one launch) -> pw2 accumulated into h
            _, x_op = self._ln(L, stream, h, lw["ln_conv"], eps=INNER_EPS, want_f32=False)
            _, u_op = self._linear(L, stream, x_op, lw["pw1"], None, want_op=True)
            a_op = self._buf(b, t, c, dtype=op_dtype)
            _lib.check(L.ts_conformer_glu_dwconv_fwd(u_op.data_ptr(), b, t, c, lw["dw"].data_ptr(), self.kdw, lw["bn_scale"].data_ptr(),
                                                     lw["bn_shift"].data_ptr(), self.act, self.prec, a_op.data_ptr(), stream),
                       "ts_conformer_glu_dwconv_fwd")
            self._linear(L, stream, a_op, lw["pw2"], None, into=h)
            ffn(lw["ffn2"], lw["ln_ffn2"])
            h, _ = self._ln(L, stream, h, lw["ln_final"], eps=INNER_EPS, want_op=False)
        h, _ = self._ln(L, stream, h, self.enc_ln, want_op=False)
        return self._adapter(L, stream, h) if self.adapter else h
