"""WavLM-large inference on the HIP path vs wav2vec2-large at the same geometry (random weights), 16 x 20 s, bf16 -- and the per-launch time of
the gated relative-position attention kernel (ts_wavlm_attention_fwd) vs the wav2vec2 one (ts_w2v_attention_fwd) at t = 999 frames.
python tools/bench_wavlm.py [--batch 16] [--seconds 20] [--layers 24] [--steps 5] [--out FILE.md]

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seconds", type=int, default=20)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the table (markdown) to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_wavlm: needs an MI355X")
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
