"""wav2vec2-conformer-large (rotary) inference on the HIP path vs wav2vec2-large pre-LN at the same geometry (random weights), 16 x 20 s, bf16,
eager and graphed -- and per-launch times at t = 999 frames, 16 clips, 1024 channels: ts_conformer_glu_dwconv_fwd, the LayerNorm + rotary launch
next to ts_w2v_layernorm_fwd, and the SiLU GEMM next to the GELU GEMM at the feed-forward shape.
python tools/bench_conformer.py [--batch 16] [--seconds 20] [--layers 24] [--steps 5] [--out profiles/conformer_forward.md]

Rows, all 1024 hidden / 16 heads / 24 layers / 4096 ffn, layer-norm conv feature extractor:
  wav2vec2-large pre-LN      tools/bench_c5.py's weights as a layer-norm / pre-LN model (tools/bench_wavlm.py layer_norm_variant)
  wav2vec2-conformer-large   conformer blocks (k = 31, swish, rotary), the same front end

python tools/bench_conformer.py --train [--batch 8] [--seconds 10] [--layers 24] [--steps 5] [--out profiles/conformer_finetune.md]
--train: mixed-precision fine-tuning steps (train_precision="bf16": training forward, backward of a probe loss, AdamW; tools/bench_wavlm.py's
time_train) of wav2vec2-conformer-large next to wav2vec2-large pre-LN at the same geometry in the same run, peak allocated memory of each, and every
launch of csrc/conformer_train.hip per call at t = 499 (3 992 rows x 1024 channels) next to its HBM floor: the bytes it must move over the 8 TB/s peak of
MI355X_MICROARCH.md (about 6.3 TB/s is achievable).  Each launch rotates through enough buffer sets to put 600 MB between two uses of a buffer, so the
256 MiB Infinity Cache does not serve the operands."""
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


def train_model(conformer: bool, layers, seed=0):
    """wav2vec2-large pre-LN (tools/bench_wavlm.py train_models' configuration) or wav2vec2-conformer-large (rotary, k = 31, swish) as a transformers
    module: random weights, dropouts 0.1 as in fine-tuning recipes.  One model per call: both at once would hold 0.9 G parameters on the host."""
    import transformers
    kw = dict(hidden_size=1024, num_hidden_layers=layers, num_attention_heads=16, intermediate_size=4096, feat_extract_norm="layer", conv_bias=True,
              hidden_dropout=0.1, attention_dropout=0.1, activation_dropout=0.1, feat_proj_dropout=0.1, layerdrop=0.0, mask_time_prob=0.05,
              mask_feature_prob=0.0, vocab_size=32)
    torch.manual_seed(seed)
    if not conformer:
        return transformers.Wav2Vec2Model(transformers.Wav2Vec2Config(**kw, do_stable_layer_norm=True))
    return transformers.Wav2Vec2ConformerModel(transformers.Wav2Vec2ConformerConfig(**kw, conformer_conv_dropout=0.1, position_embeddings_type="rotary",
                                                                                  hidden_act="swish", conv_depthwise_kernel_size=31))


def time_train_launches(b=8, t=499, c=1024, ff=4096, k=31, heads=16, reps=20, spread_mb=600):
    """{launch: (us per call, bytes it must move)}: device events, best of three alternating blocks of `reps`, rotating buffer sets."""
    from thunder_speech_amd import _lib
    from thunder_speech_amd.huggingface.conformer import rotary_table
    from thunder_speech_amd.huggingface.train import _pad32
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    rows, rp = b * t, _pad32(b * t)
    nc, nf = rows * c, rows * ff
    g = torch.Generator().manual_seed(4)
    n_sets = lambda nbytes: max(2, -(-spread_mb * 10 ** 6 // nbytes))
    f32 = lambda sets, *shape: [torch.randn(*shape, generator=g).cuda() for _ in range(sets)]
    b16 = lambda sets, *shape: [torch.empty(*shape, dtype=torch.bfloat16, device="cuda") for _ in range(sets)]
    dw = (0.2 * torch.randn(k, c, generator=g)).cuda()
    gamma, beta = (1.0 + 0.1 * torch.randn(c, generator=g)).cuda(), (0.1 * torch.randn(c, generator=g)).cuda()
    table = rotary_table(1.0 / (10000 ** (torch.arange(0, 64, 2, dtype=torch.int64).float() / 64)), 5000).cuda()
    mean_rstd, mean_var = torch.empty(2, c, device="cuda"), torch.empty(2, c, device="cuda")
    dgamma, dbeta, ddw = torch.empty(c, device="cuda"), torch.empty(c, device="cuda"), torch.empty(k, c, device="cuda")
    ws_f = torch.empty(L.ts_conformer_glu_dwconv_train_fwd_workspace(b, t, c), dtype=torch.uint8, device="cuda")
    ws_s = torch.empty(L.ts_conformer_bn_act_bwd_sums_workspace(rows, c), dtype=torch.uint8, device="cuda")
    ws_b = torch.empty(L.ts_conformer_glu_dwconv_train_bwd_workspace(b, t, c, k), dtype=torch.uint8, device="cuda")
    bias_f = torch.zeros(ff, device="cuda")
    ns = n_sets(24 * nc)                                      # the conv module's launches share their sets: sized by the largest mover
    u, z, da, du = f32(ns, b, t, 2 * c), f32(ns, b, t, c), f32(ns, b, t, c), f32(ns, b, t, 2 * c)
    a16, at16 = b16(ns, rows, c), b16(ns, c, rp)
    nr = n_sets(12 * nc)
    dv, dr, dy = f32(nr, b, t, c), f32(nr, b, t, c), f32(nr, b, t, c)
    nff = n_sets(12 * nf)
    zf, daf, dzf = f32(nff, rows, ff), f32(nff, rows, ff), f32(nff, rows, ff)
    f16, ft16 = b16(nff, rows, ff), b16(nff, ff, rp)
    # statistics and sums the backward launches read: made once, from set 0
    _lib.check(L.ts_conformer_glu_dwconv_train_fwd(u[0].data_ptr(), b, t, c, dw.data_ptr(), k, z[0].data_ptr(), ws_f.data_ptr(), s), "fwd")
    _lib.check(L.ts_conformer_bn_stats(ws_f.data_ptr(), b, t, c, 1e-5, mean_rstd.data_ptr(), mean_var.data_ptr(), s), "stats")
    calls = {
        "ts_conformer_glu_dwconv_train_fwd": (12 * nc, ns, lambda i: L.ts_conformer_glu_dwconv_train_fwd(
            u[i].data_ptr(), b, t, c, dw.data_ptr(), k, z[i].data_ptr(), ws_f.data_ptr(), s)),
        "ts_conformer_bn_stats": (ws_f.numel(), 1, lambda i: L.ts_conformer_bn_stats(ws_f.data_ptr(), b, t, c, 1e-5, mean_rstd.data_ptr(), mean_var.data_ptr(), s)),
        "ts_conformer_bn_act_cast": (4 * nc + 2 * nc + 2 * c * rp, ns, lambda i: L.ts_conformer_bn_act_cast(
            z[i].data_ptr(), mean_rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), rows, c, 2, a16[i].data_ptr(), at16[i].data_ptr(), rp, rp, s)),
        "ts_conformer_bn_act_bwd_sums": (8 * nc, ns, lambda i: L.ts_conformer_bn_act_bwd_sums(
            z[i].data_ptr(), mean_rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), da[i].data_ptr(), rows, c, 2, dgamma.data_ptr(), dbeta.data_ptr(),
            ws_s.data_ptr(), s)),
        "ts_conformer_glu_dwconv_train_bwd": (24 * nc, ns, lambda i: L.ts_conformer_glu_dwconv_train_bwd(
            u[i].data_ptr(), z[i].data_ptr(), da[i].data_ptr(), b, t, c, dw.data_ptr(), k, mean_rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
            dgamma.data_ptr(), dbeta.data_ptr(), 0, 2, du[i].data_ptr(), ddw.data_ptr(), ws_b.data_ptr(), s)),
        "ts_conformer_rotary_bwd": (12 * nc, nr, lambda i: L.ts_conformer_rotary_bwd(
            dv[i].data_ptr(), dr[i].data_ptr(), b, t, c, table.data_ptr(), 5000, dy[i].data_ptr(), s)),
        "ts_conformer_ffn_act_cast (SiLU, p 0.1, 4096 wide)": (4 * nf + 2 * nf + 2 * ff * rp, nff, lambda i: L.ts_conformer_ffn_act_cast(
            zf[i].data_ptr(), bias_f.data_ptr(), rows, ff, 2, 0.1, 7, f16[i].data_ptr(), ft16[i].data_ptr(), rp, rp, s)),
        "ts_conformer_ffn_act_bwd (SiLU, p 0.1, 4096 wide)": (12 * nf, nff, lambda i: L.ts_conformer_ffn_act_bwd(
            zf[i].data_ptr(), bias_f.data_ptr(), ff, 2, daf[i].data_ptr(), 0.1, 7, dzf[i].data_ptr(), nf, s)),
    }
    best = {name: float("inf") for name in calls}
    for _ in range(3):
        for name, (_, sets, f) in calls.items():
            _lib.check(f(0), name)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for r in range(reps):
                f(r % sets)
            e1.record(); torch.cuda.synchronize()
            best[name] = min(best[name], e0.elapsed_time(e1) / reps * 1e3)
    return {name: (best[name], calls[name][0]) for name in calls}


def main_train(a):
    from tools.bench_wavlm import time_train
    rows = []
    for name, pick in (("wav2vec2-large (layer norm, pre-LN)", False), ("wav2vec2-conformer-large (rotary, k = 31, swish)", True)):
        model = train_model(pick, a.layers)
        params = sum(p.numel() for p in model.parameters() if p.requires_grad)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        ms = time_train(name, model, a)
        rows.append((name, ms, torch.cuda.max_memory_allocated() / 2 ** 30, params))
        del model
        torch.cuda.empty_cache()
    launches = time_train_launches(b=a.batch)
    t = (16000 * a.seconds - 400) // 320 + 1
    lines = [f"fine-tuning step, train_precision=\"bf16\": {a.batch} x {a.seconds} s (one clip 3/4 long; t = {t} frames), {a.layers} layers, 1024 hidden / "
             f"16 heads / 4096 ffn, dropouts 0.1, mask_time_prob 0.05; {a.steps} timed steps after 2 warm-up steps, host clock around a device synchronise", "",
             "| model | trained parameters | ms/step | vs wav2vec2-large pre-LN | peak allocated GiB |", "|---|---:|---:|---:|---:|"]
    for name, ms, gib, params in rows:
        lines.append(f"| {name} | {params / 1e6:.0f} M | {ms:.1f} | {ms / rows[0][1]:.3f} | {gib:.2f} |")
    lines += ["", f"launches of csrc/conformer_train.hip, {a.batch} clips x t = 499 x 1024 channels, k = 31 (device events, best of 3 blocks of 20 calls, "
              "buffer sets rotated so that 600 MB lie between two uses of a buffer); floor = bytes / 8 TB/s:", "",
              "| launch | MB it must move | us per call | HBM floor us | TB/s | floor / measured |", "|---|---:|---:|---:|---:|---:|"]
    for name, (us, nbytes) in launches.items():
        floor = nbytes / 8e12 * 1e6
        lines.append(f"| {name} | {nbytes / 1e6:.1f} | {us:.1f} | {floor:.1f} | {nbytes / us / 1e6:.2f} | {floor / us:.2f} |")
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
        raise SystemExit("bench_conformer: needs an MI355X")
    if a.train:
        text = "\n".join(main_train(a))
        print(text)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text + "\n")
        return
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
