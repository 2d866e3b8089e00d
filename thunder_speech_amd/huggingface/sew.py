"""SEW encoder (transformers' SEWModel, the "squeezed and efficient" wav2vec2) on the HIP kernels of csrc/sew.hip and the wav2vec2 files
(csrc/w2v_conv.hip, w2v_rows.hip, w2v_attn.hip, gemm_nt.hip).

transformers modeling_sew.py, reached from the reference's `_HuggingFaceEncoderAdapt.forward` (huggingface/compatibility.py:31-42) for a SEW
checkpoint.  With s = config.squeeze_factor, k = config.num_conv_pos_embeddings, T frames out of the conv feature extractor and T2 = T // s:

    1. conv feature extractor: wav2vec2's (`Wav2Vec2Plan`), the layer lists include kernel-1 layers
    2. `layer_norm` over conv_dim[-1] (config.layer_norm_eps); `feature_projection` -- a plain Linear, keys feature_projection.weight / .bias --
       only when conv_dim[-1] != hidden_size
    3. with an attention mask, rows >= len are zeroed (ts_w2v_mask_rows)
    4. squeeze, one call (ts_sew_squeeze_fwd): hp[r] = mean_{i < s} h[s r + i] + gelu(conv_stride_s(h)[r] + bias) for r < T2 -- the weight-normed grouped
       conv has padding k // 2; transformers' same-pad trim and its min_length always land on T2 frames
    5. `encoder.layer_norm`, then wav2vec2's post-LN layers (`Wav2Vec2Plan._post_ln_layers`) at T2 frames; valid keys min(ceil(len / s), T2): the
       max_pool1d of transformers' mask
    6. upsample: gelu(linear C -> s C) over all B T2 rows in one GEMM, read row-major as [B][s T2][C]; zero rows up to T (ts_sew_unsqueeze_rows,
       only when T % s != 0: otherwise the GEMM's output already is the result)

This module is the inference plan; train mode runs the same six steps as autograd nodes, in mixed precision only (huggingface/sew_train.py,
csrc/sew_train.hip).  T, T2 and every buffer shape are host integers, the key lengths are computed on the device: the forward captures into a hipGraph."""
from __future__ import annotations

from typing import Dict, Optional

import torch

from .. import _lib
from .encoder import Wav2Vec2Plan, feat_extract_output_lengths

__all__ = ["SEWPlan", "pooled_key_lengths", "squeeze_on_matrix_cores", "pack_squeeze_taps"]

SQUEEZE_SLOT = 32                 # channels per group of the matrix-core kernel (24 is packed as 32)
SQUEEZE_FRAMES = 128              # its output frames per workgroup
SQUEEZE_PITCH = 144               # bytes per staged window row
SQUEEZE_LDS = 64 * 1024


def pooled_key_lengths(lengths: torch.Tensor, stride: int, t2: int) -> torch.Tensor:
    """Valid keys of the squeezed sequence for `lengths` valid frames: the number of ones in max_pool1d(mask, stride, stride), min(ceil(len / s), T2)
    (integer tensor in, out; stays on the tensor's device)."""
    return torch.clamp(torch.div(lengths + (stride - 1), stride, rounding_mode="floor"), max=t2)


def squeeze_on_matrix_cores(channels_per_group: int, kernel: int, stride: int) -> bool:
    """Whether ts_sew_squeeze_fwd(precision = 1) has its matrix-core kernel for this geometry: 24 or 32 channels per group and a staged window of
    127 stride + kernel rows (rounded up to a multiple of stride) within 64 KiB of LDS.  Python mirror of the launcher's dispatch."""
    rows = (SQUEEZE_FRAMES - 1) * stride + kernel
    return channels_per_group in (24, SQUEEZE_SLOT) and -(-rows // stride) * stride * SQUEEZE_PITCH <= SQUEEZE_LDS


def pack_squeeze_taps(w_eff: torch.Tensor, groups: int, matrix_cores: bool) -> torch.Tensor:
    """conv weight [C][C / groups][k] (weight norm applied) -> the tap layout of ts_sew_squeeze_fwd, `pos_w`'s [k][g][out][in]: f32 at the
    checkpoint's width, or (`matrix_cores`) bf16 with every [out][in] block zero-padded to 32 x 32."""
    c, cg, k = w_eff.shape
    w = w_eff.view(groups, cg, cg, k).permute(3, 0, 1, 2)
    if not matrix_cores:
        return w.contiguous()
    out = torch.zeros(k, groups, SQUEEZE_SLOT, SQUEEZE_SLOT, dtype=torch.bfloat16, device=w_eff.device)
    out[:, :, :cg, :cg] = w.to(torch.bfloat16)
    return out


class SEWPlan(Wav2Vec2Plan):
    """Packed weights + launch sequence of a SEWModel.  precision as Wav2Vec2Plan: "fp32" or "bf16" (bf16 GEMM operands, f32 accumulation, residual
    stream, normalisations, softmax and average pool).  In bf16 mode the squeeze runs on the matrix cores where that kernel exists
    (`squeeze_on_matrix_cores`); any other geometry takes the f32 path of the same call."""

    def __init__(self, cfg, sd: Dict[str, torch.Tensor], device, precision: str = "bf16"):
        # the base packs the conv feature extractor only: SEW's projection keys and positional conv are not wav2vec2's
        super().__init__(cfg, sd, device, precision, feature_extractor_only=True)
        self.feature_extractor_only = False
        f = lambda k: sd[k].detach().to(device=self.device, dtype=torch.float32).contiguous()
        gw = (lambda t: t.to(torch.bfloat16).contiguous()) if self.prec else (lambda t: t.contiguous())
        self.squeeze = int(cfg.squeeze_factor)
        self.fe_ln = (f("layer_norm.weight"), f("layer_norm.bias"))
        self.project = self.dims[-1] != self.hidden
        if self.project:
            self.fp_w, self.fp_b = gw(f("feature_projection.weight")), f("feature_projection.bias")
        p = "encoder.pos_conv_embed.conv."
        self.sq_mfma = bool(self.prec) and squeeze_on_matrix_cores(self.hidden // self.groups, self.kpos, self.squeeze)
        self.sq_prec = 1 if self.sq_mfma else 0
        self.sq_w = pack_squeeze_taps(self._weight_normed(sd, f, p), self.groups, self.sq_mfma)
        self.sq_b = f(p + "bias")
        self.enc_ln = (f("encoder.layer_norm.weight"), f("encoder.layer_norm.bias"))
        self.layers = [self._pack_layer(f, gw, f"encoder.layers.{i}.") for i in range(self.n_layers)]
        self.up_w, self.up_b = gw(f("encoder.upsample.projection.weight")), f("encoder.upsample.projection.bias")      # [s C][C]

    def forward(self, audio: torch.Tensor, lengths: Optional[torch.Tensor]) -> torch.Tensor:
        """audio [B, n] fp32 on the GPU; lengths = samples per clip with `mask_input`, else None.  -> last_hidden_state [B, T, C] fp32."""
        L = _lib.lib()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        feats, _ = self._feature_extractor(audio)
        b, t, _ = feats.shape
        c, s = self.hidden, self.squeeze
        if t < s:
            raise RuntimeError(f"sew: input too short: {t} frames behind the conv feature extractor, squeeze_factor {s}")
        t2 = t // s
        if self.project:
            _, ln_op = self._ln(L, stream, feats, self.fe_ln, want_f32=False)
            h, _ = self._linear(L, stream, ln_op, self.fp_w, self.fp_b)
        else:
            h, _ = self._ln(L, stream, feats, self.fe_ln, want_op=False)
        key_len = None
        if lengths is not None:
            frames = feat_extract_output_lengths(self.kernels, self.strides, lengths.to(self.device).long())
            key_len = pooled_key_lengths(frames, s, t2).to(torch.int32).contiguous()
            frames = frames.to(torch.int32).contiguous()
            _lib.check(L.ts_w2v_mask_rows(h.data_ptr(), b, t, c, frames.data_ptr(), stream), "ts_w2v_mask_rows")
        ws = self._buf(L.ts_sew_squeeze_workspace_bytes(b, t, c, self.kpos, s, self.sq_prec), dtype=torch.uint8)
        hp = self._buf(b, t2, c)
        _lib.check(L.ts_sew_squeeze_fwd(h.data_ptr(), b, t, c, self.sq_w.data_ptr(), self.sq_b.data_ptr(), self.kpos, self.groups, s, self.sq_prec,
                                        hp.data_ptr(), ws.data_ptr(), stream), "ts_sew_squeeze_fwd")
        del ws
        _, h_op = self._post_ln_layers(L, stream, hp, None, self._attention(L, stream, b, t2, key_len))
        up, _ = self._linear(L, stream, h_op, self.up_w, self.up_b, act=1)            # [B][T2][s C] = [B][s T2][C] row-major
        if s * t2 == t:
            return up.view(b, t, c)
        out = self._buf(b, t, c)
        _lib.check(L.ts_sew_unsqueeze_rows(up.data_ptr(), b, t2, t, c, s, out.data_ptr(), stream), "ts_sew_unsqueeze_rows")
        return out
