"""WavLM-large inference on the HIP path vs wav2vec2-large at the same geometry (random weights), 16 x 20 s, bf16 -- and the per-launch time of
the gated relative-position attention kernel (ts_wavlm_attention_fwd) vs the wav2vec2 one (ts_w2v_attention_fwd) at t = 999 frames.
python tools/bench_wavlm.py [--batch 16] [--seconds 20] [--layers 24] [--steps 5] [--out FILE.md]
python tools/bench_wavlm.py --train [--batch 8] [--seconds 10] [--layers 24] [--steps 5] [--out FILE.md]

--train: mixed-precision fine-tuning steps (train_precision="bf16": training forward, backward of a CTC-sized probe loss, AdamW) of WavLM-large
against wav2vec2-large pre-LN with the same weights (WavLM's gate and position embedding added), dropouts 0.1, and the per-launch times of the
fused training attention kernels (ts_wavlm_attention_train_fwd / _bwd vs ts_w2v_attention_train_fwd / _bwd) at the step's geometry.

Rows, all 1024 hidden / 16 heads / 24 layers / 4096 ffn:
  wav2vec2-large C5     tools/bench_c5.py's config (group norm, post-LN): the headline C5 workload
  wav2vec2-large pre-LN the same weights as a layer-norm / pre-LN model (the family of wavlm-large): the like-for-like baseline
  wavlm-large           layer norm / pre-LN + gated relative-position attention (320 buckets, max distance 800; t = 999 > 800 clamps)"""
import argparse
import os
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tools.bench_c5 import config, random_state


def layer_norm_variant(cfg, sd, wavlm: bool, seed=1):
    """cfg / state dict of the layer-norm, pre-LN family on bench_c5's weights (+ WavLM's attention gate and position embedding)."""
    cfg = SimpleNamespace(**{**vars(cfg), "feat_extract_norm": "layer", "do_stable_layer_norm": True, "model_type": "wavlm" if wavlm else "wav2vec2"})
    sd = dict(sd)
    for i in range(1, len(cfg.conv_kernel)):
        sd[f"feature_extractor.conv_layers.{i}.layer_norm.weight"] = torch.ones(cfg.conv_dim[i])
        sd[f"feature_extractor.conv_layers.{i}.layer_norm.bias"] = torch.zeros(cfg.conv_dim[i])
    if wavlm:
        cfg.num_buckets, cfg.max_bucket_distance = 320, 800
        g = torch.Generator().manual_seed(seed)
        h = cfg.num_attention_heads
        sd["encoder.layers.0.attention.rel_attn_embed.weight"] = torch.randn(320, h, generator=g)
        for i in range(cfg.num_hidden_layers):
            p = f"encoder.layers.{i}.attention."
            sd[p + "gru_rel_pos_linear.weight"] = 0.1 * torch.randn(8, 64, generator=g)
            sd[p + "gru_rel_pos_linear.bias"] = torch.zeros(8)
            sd[p + "gru_rel_pos_const"] = torch.ones(1, h, 1, 1)
    return cfg, sd


def time_model(name, cfg, sd, a):
    from thunder_speech_amd.huggingface.encoder import Wav2Vec2Plan
    from thunder_speech_amd.huggingface.transform import Wav2Vec2Preprocess
    plan = Wav2Vec2Plan(cfg, sd, "cuda", precision="bf16")
    pre = Wav2Vec2Preprocess()
    g = torch.Generator().manual_seed(0)
    x = (0.1 * torch.randn(a.batch, 16000 * a.seconds, generator=g)).cuda()
    lengths = torch.full((a.batch,), 16000 * a.seconds, dtype=torch.int32, device="cuda")

    def step():
        xn, _ = pre(x, lengths)
        return plan.forward(xn, None)

    res = {}
    with torch.no_grad():
        out = step(); out = step(); torch.cuda.synchronize()
        assert torch.isfinite(out).all(), name
        graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                gout = step()
        graph.replay(); torch.cuda.synchronize()
        if not torch.equal(gout, out):
            print(f"{name}: graph replay differs from the eager forward by {float((gout - out).abs().max()):.3g}")
        for mode, run in (("eager", step), ("graphed", graph.replay)):
            run(); torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                run()
            torch.cuda.synchronize()
            res[mode] = (time.perf_counter() - t0) / a.steps * 1e3
    del plan, graph
    torch.cuda.empty_cache()
    return res, out.shape[1]


def time_attention(a, t=999, heads=16, reps=50):
    """Per-launch device time of the two fused attention kernels on the same bf16 qkv, alternated in blocks."""
    from thunder_speech_amd import _lib
    from thunder_speech_amd.huggingface.encoder import wavlm_bucket_table
    L = _lib.lib()
    b, c = a.batch, 64 * heads
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(b, t, 3 * c, generator=g).to(torch.bfloat16).cuda()
    gx = torch.randn(b, t, c, generator=g).to(torch.bfloat16).cuda()
    wg, bg, cst = (0.1 * torch.randn(8, 64, generator=g)).cuda(), torch.zeros(8).cuda(), torch.ones(heads).cuda()
    E, table = torch.randn(320, heads, generator=g).cuda(), wavlm_bucket_table(320, 800).cuda()
    rb = torch.empty(heads, 2 * t - 1, device="cuda")
    ctx = torch.empty(b, t, c, dtype=torch.bfloat16, device="cuda")
    ws = torch.empty(1, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    _lib.check(L.ts_wavlm_rel_bias(E.data_ptr(), table.data_ptr(), 320, 800, heads, t, rb.data_ptr(), s), "ts_wavlm_rel_bias")
    calls = {
        "w2v_flash_attn_kernel (ts_w2v_attention_fwd)": lambda: L.ts_w2v_attention_fwd(qkv.data_ptr(), b, t, c, heads, None, 1, ctx.data_ptr(), ws.data_ptr(), s),
        "wavlm_flash_attn_kernel (ts_wavlm_attention_fwd)": lambda: L.ts_wavlm_attention_fwd(
            qkv.data_ptr(), b, t, c, heads, None, 1, gx.data_ptr(), c, wg.data_ptr(), bg.data_ptr(), cst.data_ptr(), rb.data_ptr(), ctx.data_ptr(), None, s),
        "wavlm_rel_bias_kernel (ts_wavlm_rel_bias)": lambda: L.ts_wavlm_rel_bias(E.data_ptr(), table.data_ptr(), 320, 800, heads, t, rb.data_ptr(), s),
    }
    best = {k: float("inf") for k in calls}
    for _ in range(3):                                  # three alternating blocks: the best block per kernel
        for k, f in calls.items():
            _lib.check(f(), k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                f()
            e1.record(); torch.cuda.synchronize()
            best[k] = min(best[k], e0.elapsed_time(e1) / reps * 1e3)
    return best


def train_models(layers, seed=0):
    """(wav2vec2-large pre-LN, wavlm-large) transformers modules with the same shared weights, dropouts 0.1 as in fine-tuning recipes."""
    import transformers
    kw = dict(hidden_size=1024, num_hidden_layers=layers, num_attention_heads=16, intermediate_size=4096, feat_extract_norm="layer",
              do_stable_layer_norm=True, conv_bias=True, hidden_dropout=0.1, attention_dropout=0.1, activation_dropout=0.1, feat_proj_dropout=0.1,
              layerdrop=0.0, mask_time_prob=0.05, mask_feature_prob=0.0, vocab_size=32)
    torch.manual_seed(seed)
    w2v = transformers.Wav2Vec2Model(transformers.Wav2Vec2Config(**kw))
    wl = transformers.WavLMModel(transformers.WavLMConfig(**kw, num_buckets=320, max_bucket_distance=800))
    missing = wl.load_state_dict(w2v.state_dict(), strict=False).missing_keys
    assert all("rel_attn_embed" in k or "gru_rel_pos" in k for k in missing), missing
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in wl.named_parameters():
            if n.endswith("rel_attn_embed.weight"):
                p.copy_(torch.randn(p.shape, generator=g))
            elif n.endswith("gru_rel_pos_linear.weight"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    return w2v, wl


def time_train(name, model, a):
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    adapt = HuggingFaceEncoderAdapt(model, mask_input=True, train_precision="bf16").cuda().train()
    opt = torch.optim.AdamW([p for p in adapt.parameters() if p.requires_grad], lr=1e-5)
    g = torch.Generator().manual_seed(0)
    x = (0.1 * torch.randn(a.batch, 16000 * a.seconds, generator=g)).cuda()
    lengths = torch.full((a.batch,), 16000 * a.seconds, dtype=torch.int64, device="cuda")
    lengths[-1] = 16000 * a.seconds * 3 // 4                                  # one ragged clip
    probe = None

    def step():
        nonlocal probe
        opt.zero_grad(set_to_none=True)
        feats, _ = adapt(x, lengths)
        if probe is None:
            probe = torch.randn(feats.shape, generator=g).cuda()
        (feats * probe).mean().backward()
        opt.step()

    for _ in range(2):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / a.steps * 1e3
    del adapt, opt
    torch.cuda.empty_cache()
    return ms


def time_train_attention(a, t, heads=16, p=0.1, reps=20):
    """Per-launch device time of the fused training attention, forward and backward, WavLM vs wav2vec2, alternated in blocks."""
    from thunder_speech_amd import _lib
    from thunder_speech_amd.huggingface.encoder import wavlm_bucket_table
    L = _lib.lib()
    b, c = a.batch, 64 * heads
    g = torch.Generator().manual_seed(3)
    q16 = torch.randn(b, t, 3 * c, generator=g).to(torch.bfloat16).cuda()
    gate = (1.0 + torch.rand(b, heads, t, generator=g)).cuda()
    E, table = torch.randn(320, heads, generator=g).cuda(), wavlm_bucket_table(320, 800).cuda()
    rb = torch.empty(heads, 2 * t - 1, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    _lib.check(L.ts_wavlm_rel_bias(E.data_ptr(), table.data_ptr(), 320, 800, heads, t, rb.data_ptr(), s), "ts_wavlm_rel_bias")
    dout = torch.randn(b, t, c, generator=g).cuda()
    ctx, lse2 = torch.empty(b, t, c, device="cuda"), torch.empty(b, heads, t, device="cuda")
    ctx2, lse22 = torch.empty_like(ctx), torch.empty_like(lse2)
    dq, dq2 = torch.empty(b, t, 3 * c, device="cuda"), torch.empty(b, t, 3 * c, device="cuda")
    dg, drb = torch.empty_like(gate), torch.empty_like(rb)
    wf = torch.empty(L.ts_w2v_attention_train_fwd_workspace(b, t, c, heads), dtype=torch.uint8, device="cuda")
    wf2 = torch.empty(L.ts_wavlm_attention_train_fwd_workspace(b, t, c, heads), dtype=torch.uint8, device="cuda")
    wb = torch.empty(L.ts_w2v_attention_train_bwd_workspace(b, t, c, heads), dtype=torch.uint8, device="cuda")
    wb2 = torch.empty(L.ts_wavlm_attention_train_bwd_workspace(b, t, c, heads), dtype=torch.uint8, device="cuda")
    calls = {
        "ts_w2v_attention_train_fwd": lambda: L.ts_w2v_attention_train_fwd(q16.data_ptr(), b, t, c, heads, None, p, 7, ctx.data_ptr(), lse2.data_ptr(),
                                                                           wf.data_ptr(), s),
        "ts_wavlm_attention_train_fwd": lambda: L.ts_wavlm_attention_train_fwd(q16.data_ptr(), b, t, c, heads, None, p, 7, gate.data_ptr(), rb.data_ptr(),
                                                                               ctx2.data_ptr(), lse22.data_ptr(), wf2.data_ptr(), s),
        "ts_w2v_attention_train_bwd": lambda: L.ts_w2v_attention_train_bwd(q16.data_ptr(), b, t, c, heads, None, p, 7, dout.data_ptr(), ctx.data_ptr(),
                                                                           lse2.data_ptr(), wf.data_ptr(), dq.data_ptr(), wb.data_ptr(), s),
        "ts_wavlm_attention_train_bwd": lambda: L.ts_wavlm_attention_train_bwd(q16.data_ptr(), b, t, c, heads, None, p, 7, gate.data_ptr(), rb.data_ptr(),
                                                                               dout.data_ptr(), ctx2.data_ptr(), lse22.data_ptr(), wf2.data_ptr(),
                                                                               dq2.data_ptr(), dg.data_ptr(), drb.data_ptr(), wb2.data_ptr(), s),
    }
    best = {k: float("inf") for k in calls}
    for _ in range(3):
        for k, f in calls.items():
            _lib.check(f(), k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                f()
            e1.record(); torch.cuda.synchronize()
            best[k] = min(best[k], e0.elapsed_time(e1) / reps * 1e3)
    ws_mb = L.ts_wavlm_attention_train_bwd_workspace(b, t, c, heads) / 2 ** 20
    return best, ws_mb


def main_train(a):
    w2v, wl = train_models(a.layers)
    t = None
    rows = []
    for name, m in (("wav2vec2-large (layer norm, pre-LN)", w2v), ("wavlm-large (layer norm, pre-LN)", wl)):
        rows.append((name, time_train(name, m, a)))
    from thunder_speech_amd.huggingface.encoder import feat_extract_output_lengths
    t = int(feat_extract_output_lengths(w2v.config.conv_kernel, w2v.config.conv_stride, torch.tensor([16000 * a.seconds]))[0])
    del w2v, wl
    att, ws_mb = time_train_attention(a, t)
    base = rows[0][1]
    lines = [f"fine-tuning step, train_precision=\"bf16\": {a.batch} x {a.seconds} s (one clip 3/4 long), {a.layers} layers, 1024 hidden / 16 heads, "
             f"t = {t} frames, dropouts 0.1, mask_time_prob 0.05; forward + backward + AdamW, {a.steps} timed steps after 2 warm-up steps",
             "", "| model | ms/step | vs wav2vec2-large pre-LN |", "|---|---:|---:|"]
    for name, ms in rows:
        lines.append(f"| {name} | {ms:.1f} | {ms / base:.3f} |")
    lines += ["", f"fused training attention, {a.batch} clips x 16 heads x t = {t}, p = 0.1 (device events, best of 3 blocks of 20):", "",
              "| entry point | us per call | vs wav2vec2 |", "|---|---:|---:|"]
    for k, us in att.items():
        ref = att[k.replace("wavlm", "w2v")]
        lines.append(f"| {k} | {us:.1f} | {us / ref:.3f} |")
    lines += ["", f"ts_wavlm_attention_train_bwd workspace at this geometry: {ws_mb:.1f} MiB"]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=None, help="default 16 (inference), 8 (--train)")
    ap.add_argument("--seconds", type=int, default=None, help="default 20 (inference), 10 (--train)")
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--train", action="store_true", help="mixed-precision fine-tuning steps instead of inference")
    ap.add_argument("--out", default=None, help="also write the table (markdown) to this file")
    a = ap.parse_args()
    a.batch = a.batch or (8 if a.train else 16)
    a.seconds = a.seconds or (10 if a.train else 20)
    if not torch.cuda.is_available():
        raise SystemExit("bench_wavlm: needs an MI355X")
    if a.train:
        text = "\n".join(main_train(a))
        print(text)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text + "\n")
        return
    cfg = config(False, a.layers)
    sd = random_state(cfg)
    rows, t = [], None
    for name, (c, s) in (("wav2vec2-large C5 (group norm, post-LN)", (cfg, sd)),
                         ("wav2vec2-large (layer norm, pre-LN)", layer_norm_variant(cfg, sd, False)),
                         ("wavlm-large (layer norm, pre-LN)", layer_norm_variant(cfg, sd, True))):
        r, t = time_model(name, c, s, a)
        rows.append((name, r))
    att = time_attention(a)
    base = rows[1][1]
    lines = [f"{a.batch} x {a.seconds} s, {a.layers} layers, 1024 hidden / 16 heads, bf16, t = {t} frames; {a.steps} timed steps per mode after warm-up",
             "", "| model | eager ms/step | graphed ms/step | graphed vs wav2vec2-large pre-LN |", "|---|---:|---:|---:|"]
    for name, r in rows:
        lines.append(f"| {name} | {r['eager']:.1f} | {r['graphed']:.1f} | {r['graphed'] / base['graphed']:.3f} |")
    w2v_k = att["w2v_flash_attn_kernel (ts_w2v_attention_fwd)"]
    lines += ["", f"attention launch, {a.batch} clips x 16 heads x t = 999 (device events, best of 3 blocks of 50):", "",
              "| kernel | us per launch | vs w2v_flash_attn_kernel |", "|---|---:|---:|"]
    for k, us in att.items():
        lines.append(f"| {k} | {us:.1f} | {us / w2v_k:.3f} |")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
