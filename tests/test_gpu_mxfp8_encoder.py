"""precision="mxfp8" end to end: Wav2Vec2Plan and HuggingFaceEncoderAdapt on three geometries against the "bf16" plan of the same weights, the f32
oracle (oracle/w2v.py) and its fake-quantised restatement (tests/mxfp8_restatement.py: both operands of the four products of every transformer
layer through bf16 and the MX quantiser, everything else f32).

Per geometry, q = rms(fake-quantised restatement - f32 oracle) is computed here on the CPU, and
  rms(y_mxfp8 - y_bf16) <= 2 q      the two plans share their bf16 front bit for bit, so the difference is the quantisation effect; two quantised
                                    evaluations that differ by upstream rounding decorrelate, hence the factor 2
  rms(y_mxfp8 - y_bf16) >= q / 4    the quantised path ran, not the bf16 one
  rms(y_mxfp8 - f32 oracle) <= 2 q + 0.01   (0.01: the bf16 mode's rms tolerance on the unit-scale output, tests/test_gpu_w2v_encoder.py)
The weights are seeded random (or the transformers-generated fixture's): the figures say nothing about a trained checkpoint's transcripts."""
import functools
from types import SimpleNamespace

import pytest
import torch
from torch import nn

from mxfp8_restatement import w2v_forward_fake_quant
from oracle import w2v as ow
from test_gpu_w2v_encoder import _hf_cfg
from test_oracle_w2v import load_fixture

gpu = pytest.mark.gpu


def _random_sd(cfg: ow.W2VConfig, seed: int):
    """HF state dict of a wav2vec2 with seeded random weights at unit-scale activations (weights N(0, 1 / fan_in), LayerNorm gains near 1)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    lin = lambda n, k: (rn(n, k) / k ** 0.5, 0.1 * rn(n))
    ln = lambda c: (1.0 + 0.1 * rn(c), 0.1 * rn(c))
    sd = {}
    c_in = 1
    for i, (c, k) in enumerate(zip(cfg.conv_dim, cfg.conv_kernel)):
        p = f"feature_extractor.conv_layers.{i}."
        sd[p + "conv.weight"] = rn(c, c_in, k) * (2.0 / (c_in * k)) ** 0.5
        if cfg.conv_bias:
            sd[p + "conv.bias"] = 0.1 * rn(c)
        if cfg.feat_extract_norm == "layer" or i == 0:
            sd[p + "layer_norm.weight"], sd[p + "layer_norm.bias"] = ln(c)
        c_in = c
    h, groups, kpos = cfg.hidden_size, cfg.num_conv_pos_embedding_groups, cfg.num_conv_pos_embeddings
    sd["feature_projection.layer_norm.weight"], sd["feature_projection.layer_norm.bias"] = ln(c_in)
    sd["feature_projection.projection.weight"], sd["feature_projection.projection.bias"] = lin(h, c_in)
    sd["encoder.pos_conv_embed.conv.weight_v"] = 0.05 * rn(h, h // groups, kpos)
    sd["encoder.pos_conv_embed.conv.weight_g"] = 0.5 + 0.1 * rn(1, 1, kpos).abs()
    sd["encoder.pos_conv_embed.conv.bias"] = 0.1 * rn(h)
    sd["encoder.layer_norm.weight"], sd["encoder.layer_norm.bias"] = ln(h)
    for i in range(cfg.num_hidden_layers):
        p = f"encoder.layers.{i}."
        for name in ("q_proj", "k_proj", "v_proj", "out_proj"):
            sd[p + f"attention.{name}.weight"], sd[p + f"attention.{name}.bias"] = lin(h, h)
        sd[p + "layer_norm.weight"], sd[p + "layer_norm.bias"] = ln(h)
        sd[p + "feed_forward.intermediate_dense.weight"], sd[p + "feed_forward.intermediate_dense.bias"] = lin(cfg.intermediate_size, h)
        sd[p + "feed_forward.output_dense.weight"], sd[p + "feed_forward.output_dense.bias"] = lin(h, cfg.intermediate_size)
        sd[p + "final_layer_norm.weight"], sd[p + "final_layer_norm.bias"] = ln(h)
    return sd


def _geometry(name):
    """(oracle config, state dict, audio [B][n], lengths [B])"""
    z, sd, mid = load_fixture("w2v_mid.npz")
    if name == "w2v_mid":
        return mid, sd, torch.from_numpy(z["x"]), torch.from_numpy(z["lengths"])
    front = dict(conv_dim=mid.conv_dim, conv_kernel=mid.conv_kernel, conv_stride=mid.conv_stride, num_conv_pos_embeddings=mid.num_conv_pos_embeddings)
    if name == "pre_ln_128":
        cfg = ow.W2VConfig(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, num_conv_pos_embedding_groups=2,
                           do_stable_layer_norm=True, **front)
    else:                                           # post-LN at head_dim 80: XLS-R 1B's attention geometry at a tenth of its width
        cfg = ow.W2VConfig(hidden_size=640, num_hidden_layers=2, num_attention_heads=8, intermediate_size=1280, num_conv_pos_embedding_groups=10,
                           **front)
    x = torch.randn(2, 16000, generator=torch.Generator().manual_seed(len(name)))
    return cfg, _random_sd(cfg, 11 * len(name)), x, torch.tensor([16000, 11111])


GEOMETRIES = ["w2v_mid", "pre_ln_128", "post_ln_hd80"]


@functools.lru_cache(maxsize=None)
def _case(name):
    """Everything a geometry's tests share, computed once: inputs, the f32 oracle, q, and both plans' outputs (masked by the ragged lengths)."""
    from thunder_speech_amd.huggingface.encoder import Wav2Vec2Plan
    cfg, sd, x, lengths = _geometry(name)
    xm = x * (torch.arange(x.shape[1])[None, :] < lengths[:, None])
    ref, key_len = ow.forward(cfg, sd, xm, lengths)
    fq, _ = w2v_forward_fake_quant(cfg, sd, xm, lengths)
    out = {}
    for precision in ("bf16", "mxfp8"):
        plan = Wav2Vec2Plan(_hf_cfg(cfg), sd, "cuda", precision=precision)
        out[precision] = plan.forward(xm.cuda(), lengths.cuda()).cpu()
        out[precision + "_unmasked"] = plan.forward(x.cuda(), None).cpu()
        if precision == "mxfp8":
            assert plan.mx and all(not isinstance(lw[n], torch.Tensor) for lw in plan.layers for n in ("wqkv", "wo", "w1", "w2")), \
                "the plan keeps a dense copy of a quantised weight"
    torch.cuda.synchronize()
    rms = lambda a, b: float((a.double() - b.double()).pow(2).mean().sqrt())
    return SimpleNamespace(cfg=cfg, sd=sd, x=x, xm=xm, lengths=lengths, ref=ref, key_len=key_len, q=rms(fq, ref), out=out, rms=rms)


@gpu
@pytest.mark.parametrize("name", GEOMETRIES)
def test_mxfp8_differs_from_bf16_by_the_quantisation_effect(name):
    c = _case(name)
    d = c.rms(c.out["mxfp8"], c.out["bf16"])
    e32 = c.rms(c.out["mxfp8"], c.ref)
    print(f"[mxfp8] {name}: q = {c.q:.3e}, rms(mxfp8 - bf16) = {d:.3e}, rms(mxfp8 - f32 oracle) = {e32:.3e}, "
          f"rms(bf16 - f32 oracle) = {c.rms(c.out['bf16'], c.ref):.3e}")
    assert 1e-4 < c.q < 0.1
    assert d <= 2 * c.q, (d, c.q)
    assert d >= c.q / 4, (d, c.q)
    assert e32 <= 2 * c.q + 0.01, (e32, c.q)
    assert bool(torch.isfinite(c.out["mxfp8"]).all())


@gpu
@pytest.mark.parametrize("name", GEOMETRIES)
def test_lengths_and_masked_rows_behave_as_in_bf16(name):
    """Same shapes as "bf16" with and without lengths; the 2 q bound against "bf16" holds on the valid frames alone and
    without lengths, and the frames beyond a clip's length stay as close to the f32 oracle as the whole output has to."""
    c = _case(name)
    mx, bf = c.out["mxfp8"], c.out["bf16"]
    assert mx.shape == bf.shape == c.ref.shape and c.out["mxfp8_unmasked"].shape == c.out["bf16_unmasked"].shape == bf.shape
    valid = torch.arange(mx.shape[1])[None, :] < c.key_len[:, None]
    assert 0 < int((~valid).sum()) < valid.numel()
    assert c.rms(mx[valid], bf[valid]) <= 2 * c.q
    assert c.rms(mx[~valid], c.ref[~valid]) <= 2 * c.q + 0.01                      # the frames beyond a clip's length: as the whole output
    assert c.rms(c.out["mxfp8_unmasked"], c.out["bf16_unmasked"]) <= 2 * c.q
    assert not torch.equal(c.out["mxfp8_unmasked"][1], mx[1])                       # the lengths reached the attention


class _Node(nn.Module):
    pass


def _module_from_state_dict(sd, config):
    """A module tree with the state dict's keys as frozen parameters and `config`: what HuggingFaceEncoderAdapt needs of a transformers model."""
    root = _Node()
    root.config = config
    for key, value in sd.items():
        node = root
        *path, leaf = key.split(".")
        for p in path:
            if not hasattr(node, p):
                node.add_module(p, _Node())
            node = getattr(node, p)
        node.register_parameter(leaf, nn.Parameter(value.clone(), requires_grad=False))
    return root


@gpu
def test_flipping_the_adapters_precision_repacks_the_plan():
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    c = _case("pre_ln_128")
    enc = HuggingFaceEncoderAdapt(_module_from_state_dict(c.sd, _hf_cfg(c.cfg)).cuda(), mask_input=True, precision="mxfp8").eval()
    got = {}
    with torch.no_grad():
        for step, precision in enumerate(["mxfp8", "bf16", "mxfp8", "bf16"]):
            enc.precision = precision
            y, out_len = enc(c.xm.cuda(), c.lengths.cuda())
            assert torch.equal(out_len.cpu(), c.key_len)
            got[step] = y.transpose(-1, -2).cpu()
    assert torch.equal(got[0], c.out["mxfp8"]) and torch.equal(got[2], got[0])
    assert torch.equal(got[1], c.out["bf16"]) and torch.equal(got[3], got[1])
    assert not torch.equal(got[0], got[1])


@gpu
def test_refused_configurations_raise_by_name_at_plan_construction():
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt, Wav2Vec2Plan
    c = _case("pre_ln_128")
    hf = _hf_cfg(c.cfg)
    wavlm = SimpleNamespace(**{**vars(hf), "model_type": "wavlm", "num_buckets": 320, "max_bucket_distance": 800})
    with pytest.raises(NotImplementedError, match="wavlm"):
        Wav2Vec2Plan(wavlm, c.sd, "cuda", precision="mxfp8")
    h192 = SimpleNamespace(**{**vars(hf), "hidden_size": 192, "num_attention_heads": 3, "intermediate_size": 384})
    with pytest.raises(NotImplementedError, match="hidden_size=192"):
        Wav2Vec2Plan(h192, c.sd, "cuda", precision="mxfp8")
    with pytest.raises(NotImplementedError, match="wavlm"):
        HuggingFaceEncoderAdapt(_module_from_state_dict({}, wavlm), precision="mxfp8")
    # the frozen front of the training path runs "mxfp8" as "bf16", for any family
    fe = {k: v for k, v in c.sd.items() if k.startswith("feature_extractor.")}
    front = Wav2Vec2Plan(wavlm, fe, "cuda", precision="mxfp8", feature_extractor_only=True)
    ref = Wav2Vec2Plan(hf, fe, "cuda", precision="bf16", feature_extractor_only=True)
    assert not front.mx and torch.equal(front.feature_extractor(c.x.cuda()), ref.feature_extractor(c.x.cuda()))
