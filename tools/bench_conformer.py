"""wav2vec2-conformer-large (rotary) inference on the HIP path vs wav2vec2-large pre-LN at the same geometry (random weights), 16 x 20 s, bf16,
eager and graphed -- and per-launch times at t = 999 frames, 16 clips, 1024 channels: ts_conformer_glu_dwconv_fwd, the LayerNorm + rotary launch
next to ts_w2v_layernorm_fwd, and the SiLU GEMM next to the GELU GEMM at the feed-forward shape.
python tools/bench_conformer.py [--batch 16] [--seconds 20] [--layers 24] [--steps 5] [--out profiles/conformer_forward.md]

Rows, all 1024 hidden / 16 heads / 24 layers / 4096 ffn, layer-norm conv feature extractor:
  wav2vec2-large pre-LN      tools/bench_c5.py's weights as a layer-norm / pre-LN model (tools/bench_wavlm.py layer_norm_variant)
  wav2vec2-conformer-large   conformer blocks (k = 31, swish, rotary), the same front end"""
import argparse
import os
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tools.bench_c5 import config, random_state
from tools.bench_wavlm import layer_norm_variant

EXPECTED = """Expected before measuring (from shapes): a conformer layer does 23 c^2 GEMM multiply-adds per frame against wav2vec2's 12 c^2 (1.92x); GEMMs
are ~70 % of the 17.2 ms wav2vec2-large pre-LN step, so a graphed conformer-large step of ~30-31 ms (~1.8x): GEMMs ~23 ms, attention
unchanged ~2.4 ms, five LayerNorm launches per layer ~3.8 ms, depthwise ~0.5 ms, minus the positional conv ~0.5 ms.  glu_dwconv at 16 x 999 x
1024 bf16 moves ~98 MB: <= 25 us at >= 4 TB/s.  LN + rotary writes one more bf16 copy than the plain LayerNorm: <= 1.4x ts_w2v_layernorm_fwd."""


def conformer_variant(cfg, sd, seed=2, kernel=31):
    """cfg / state dict of a rotary wav2vec2-conformer on bench_c5's front end and attention / feed-forward weights."""
    cfg = SimpleNamespace(**{**vars(cfg), "feat_extract_norm": "layer", "model_type": "wav2vec2-conformer", "hidden_act": "swish",
                             "position_embeddings_type": "rotary", "conv_depthwise_kernel_size": kernel, "max_source_positions": 5000})
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, scale=0.02: torch.randn(*s, generator=g) * scale
    c, ff = cfg.hidden_size, cfg.intermediate_size
    out = {k: v for k, v in sd.items() if not k.startswith("encoder.layers.")}
    for i in range(1, len(cfg.conv_kernel)):
        out[f"feature_extractor.conv_layers.{i}.layer_norm.weight"] = torch.ones(cfg.conv_dim[i])
        out[f"feature_extractor.conv_layers.{i}.layer_norm.bias"] = torch.zeros(cfg.conv_dim[i])
    out["encoder.embed_positions.inv_freq"] = 1.0 / (10000 ** (torch.arange(0, 64, 2, dtype=torch.int64).float() / 64))
    for i in range(cfg.num_hidden_layers):
        p = f"encoder.layers.{i}."
        for n in ("ffn1_layer_norm", "self_attn_layer_norm", "conv_module.layer_norm", "ffn2_layer_norm", "final_layer_norm"):
            out[p + n + ".weight"], out[p + n + ".bias"] = torch.ones(c), torch.zeros(c)
        for n in ("ffn1", "ffn2"):
            out[p + n + ".intermediate_dense.weight"], out[p + n + ".intermediate_dense.bias"] = r(ff, c), torch.zeros(ff)
            out[p + n + ".output_dense.weight"], out[p + n + ".output_dense.bias"] = r(c, ff), torch.zeros(c)
        for n in ("q", "k", "v", "out"):
            out[p + f"self_attn.linear_{n}.weight"], out[p + f"self_attn.linear_{n}.bias"] = r(c, c), torch.zeros(c)
        m = p + "conv_module."
        out[m + "pointwise_conv1.weight"], out[m + "pointwise_conv2.weight"] = r(2 * c, c, 1), r(c, c, 1)
        out[m + "depthwise_conv.weight"] = r(c, 1, kernel, scale=0.2)
        out[m + "batch_norm.weight"], out[m + "batch_norm.bias"] = torch.ones(c), torch.zeros(c)
        out[m + "batch_norm.running_mean"], out[m + "batch_norm.running_var"] = torch.zeros(c), torch.ones(c)
    return cfg, out


def time_model(name, plan, a):
    from thunder_speech_amd.huggingface.transform import Wav2Vec2Preprocess
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
    del graph
    torch.cuda.empty_cache()
    return res, out.shape[1]


def time_launches(a, t=999, c=1024, heads=16, ff=4096, reps=50):
    """Per-launch device time (events, best of three alternating blocks of `reps`)."""
    from thunder_speech_amd import _lib
    from thunder_speech_amd.huggingface.conformer import rotary_table
    L = _lib.lib()
    b = a.batch
    rows = b * t
    g = torch.Generator().manual_seed(4)
    s = torch.cuda.current_stream().cuda_stream
    u = torch.randn(b, t, 2 * c, generator=g).to(torch.bfloat16).cuda()
    dw, sc, sh = (0.2 * torch.randn(31, c, generator=g)).cuda(), torch.ones(c).cuda(), torch.zeros(c).cuda()
    y = torch.empty(b, t, c, dtype=torch.bfloat16, device="cuda")
    yr = torch.empty_like(y)
    h = torch.randn(b, t, c, generator=g).cuda()
    w1, b1 = torch.ones(c).cuda(), torch.zeros(c).cuda()
    table = rotary_table(1.0 / (10000 ** (torch.arange(0, 64, 2, dtype=torch.int64).float() / 64)), 5000).cuda()
    x16 = torch.randn(rows, c, generator=g).to(torch.bfloat16).cuda()
    wf = (0.02 * torch.randn(ff, c, generator=g)).to(torch.bfloat16).cuda()
    frag = torch.empty_like(wf)
    _lib.check(L.ts_gemm_nt_pack_w(wf.data_ptr(), c, ff, c, frag.data_ptr(), s), "ts_gemm_nt_pack_w")
    f_op = torch.empty(rows, ff, dtype=torch.bfloat16, device="cuda")
    bf = torch.zeros(ff, device="cuda")
    calls = {
        "ts_conformer_glu_dwconv_fwd (k = 31, swish)": lambda: L.ts_conformer_glu_dwconv_fwd(u.data_ptr(), b, t, c, dw.data_ptr(), 31, sc.data_ptr(),
                                                                                            sh.data_ptr(), 2, 1, y.data_ptr(), s),
        "ts_w2v_layernorm_fwd (bf16 copy only)": lambda: L.ts_w2v_layernorm_fwd(h.data_ptr(), None, None, w1.data_ptr(), b1.data_ptr(), 1e-5, rows, c, 0,
                                                                                None, y.data_ptr(), s),
        "ts_conformer_layernorm_rotary_fwd": lambda: L.ts_conformer_layernorm_rotary_fwd(h.data_ptr(), w1.data_ptr(), b1.data_ptr(), 1e-5, b, t, c, heads,
                                                                                        table.data_ptr(), 5000, 1, y.data_ptr(), yr.data_ptr(), s),
        "FFN GEMM 1024 -> 4096, GELU epilogue": lambda: L.ts_conformer_linear_fwd(x16.data_ptr(), c, wf.data_ptr(), frag.data_ptr(), bf.data_ptr(), None,
                                                                                  0, None, 0, f_op.data_ptr(), ff, rows, ff, c, 1, 1, s),
        "FFN GEMM 1024 -> 4096, SiLU epilogue": lambda: L.ts_conformer_linear_fwd(x16.data_ptr(), c, wf.data_ptr(), frag.data_ptr(), bf.data_ptr(), None,
                                                                                  0, None, 0, f_op.data_ptr(), ff, rows, ff, c, 2, 1, s),
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
        raise SystemExit("bench_conformer: needs an MI355X")
    from thunder_speech_amd.huggingface.conformer import ConformerPlan
    from thunder_speech_amd.huggingface.encoder import Wav2Vec2Plan
    cfg = config(False, a.layers)
    sd = random_state(cfg)
    rows, t = [], None
    for name, make in (("wav2vec2-large (layer norm, pre-LN)", lambda: Wav2Vec2Plan(*layer_norm_variant(cfg, sd, False), "cuda", precision="bf16")),
                       ("wav2vec2-conformer-large (rotary, k = 31, swish)", lambda: ConformerPlan(*conformer_variant(cfg, sd), "cuda", precision="bf16"))):
        plan = make()
        r, t = time_model(name, plan, a)
        del plan
        torch.cuda.empty_cache()
        rows.append((name, r))
    launches = time_launches(a)
    base = rows[0][1]
    lines = [EXPECTED, "", f"Measured: {a.batch} x {a.seconds} s, {a.layers} layers, 1024 hidden / 16 heads / 4096 ffn, bf16, t = {t} frames; "
             f"{a.steps} timed steps per mode after warm-up", "",
             "| model | eager ms/step | graphed ms/step | graphed vs wav2vec2-large pre-LN |", "|---|---:|---:|---:|"]
    for name, r in rows:
        lines.append(f"| {name} | {r['eager']:.1f} | {r['graphed']:.1f} | {r['graphed'] / base['graphed']:.3f} |")
    ln = launches["ts_w2v_layernorm_fwd (bf16 copy only)"]
    gelu = launches["FFN GEMM 1024 -> 4096, GELU epilogue"]
    lines += ["", f"launches, {a.batch} clips x t = 999 x 1024 channels (device events, best of 3 blocks of 50):", "",
              "| launch | us per launch | ratio |", "|---|---:|---:|"]
    for k, us in launches.items():
        ratio = us / ln if "layernorm" in k else (us / gelu if "GEMM" in k else float("nan"))
        lines.append(f"| {k} | {us:.1f} | {ratio:.3f} |" if ratio == ratio else f"| {k} | {us:.1f} | |")
    gd = launches["ts_conformer_glu_dwconv_fwd (k = 31, swish)"]
    mb = a.batch * 999 * 1024 * 3 * 2 / 1e6
    lines += ["", f"glu_dwconv moves {mb:.0f} MB: {mb / gd:.2f} TB/s."]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
