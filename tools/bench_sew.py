"""SEW inference on the HIP path next to wav2vec2-base geometry in the same run (random weights), 16 x 20 s, bf16, eager and graphed -- and
per-launch times at t = 999 frames, 16 clips: ts_sew_squeeze_fwd on the matrix cores (precision 1) against the same call on the f32 path
(precision 0), alternating in one run, and the upsampler's two launches.
python tools/bench_sew.py [--batch 16] [--seconds 20] [--layers 24] [--steps 5] [--out profiles/sew_forward.md]

The geometry arguments default to asapp/sew-mid-100k AS RECALLED, NOT VERIFIED against the published config.json (nothing can be downloaded where
this was written): hidden 512, 8 heads, 24 layers, ffn 2048, 128 positional taps in 16 groups, squeeze_factor 2, and transformers' default 13-layer
SEW feature extractor (total stride 320).  Pass the real numbers if they differ.

python tools/bench_sew.py --train [--batch 8] [--seconds 10] [--steps 5] [--out profiles/sew_finetune.md]
--train: mixed-precision fine-tuning steps (train_precision="bf16": training forward, backward of a probe loss, AdamW; tools/bench_wavlm.py's
time_train) of the same SEW geometry next to the wav2vec2-base geometry in the same run, peak allocated memory of each, and the three launches of
csrc/sew_train.hip per call at 16 clips x t = 999 next to ts_sew_squeeze_fwd on the same tensors and next to their computed floors (the conv's FLOPs
at the matrix-core rate, the bytes each call must move at the HBM rate)."""
import argparse
import os
import sys
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tools.bench_c5 import config, random_state
from tools.bench_conformer import time_model

# transformers' SEWConfig defaults: thirteen layers, kernel-1 / stride-1 layers between the strided ones
SEW_CONV_DIM = (64, 128, 128, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512)
SEW_CONV_STRIDE = (5, 2, 1, 2, 1, 2, 1, 2, 1, 2, 1, 2, 1)
SEW_CONV_KERNEL = (10, 3, 1, 3, 1, 3, 1, 3, 1, 2, 1, 2, 1)

# peaks: MI355X spec 2.5 PFLOP/s dense bf16 and 8.0 TB/s HBM3E (6.29 TB/s measured with a float4 copy)
PEAK_BF16, PEAK_HBM, COPY_HBM = 2.5e15, 8.0e12, 6.29e12


def sew_config(a):
    return SimpleNamespace(model_type="sew", conv_dim=SEW_CONV_DIM, conv_kernel=SEW_CONV_KERNEL, conv_stride=SEW_CONV_STRIDE, hidden_size=a.hidden,
                           num_hidden_layers=a.layers, num_attention_heads=a.heads, intermediate_size=a.ffn, num_conv_pos_embeddings=a.taps,
                           num_conv_pos_embedding_groups=a.groups, squeeze_factor=a.squeeze, layer_norm_eps=1e-5, feat_extract_norm="group",
                           conv_bias=False, hidden_act="gelu", feat_extract_activation="gelu")


def sew_random_state(cfg, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, scale=0.02: torch.randn(*s, generator=g) * scale
    dims, c, s = cfg.conv_dim, cfg.hidden_size, cfg.squeeze_factor
    sd = {"feature_extractor.conv_layers.0.conv.weight": r(dims[0], 1, cfg.conv_kernel[0], scale=0.3),
          "feature_extractor.conv_layers.0.layer_norm.weight": torch.ones(dims[0]), "feature_extractor.conv_layers.0.layer_norm.bias": torch.zeros(dims[0])}
    for i, k in enumerate(cfg.conv_kernel[1:], start=1):
        sd[f"feature_extractor.conv_layers.{i}.conv.weight"] = r(dims[i], dims[i - 1], k, scale=(2.0 / (dims[i - 1] * k)) ** 0.5)
    sd.update({"layer_norm.weight": torch.ones(dims[-1]), "layer_norm.bias": torch.zeros(dims[-1])})
    if dims[-1] != c:
        sd.update({"feature_projection.weight": r(c, dims[-1]), "feature_projection.bias": torch.zeros(c)})
    sd.update({"encoder.pos_conv_embed.conv.weight_g": torch.ones(1, 1, cfg.num_conv_pos_embeddings),
               "encoder.pos_conv_embed.conv.weight_v": r(c, c // cfg.num_conv_pos_embedding_groups, cfg.num_conv_pos_embeddings),
               "encoder.pos_conv_embed.conv.bias": torch.zeros(c), "encoder.layer_norm.weight": torch.ones(c), "encoder.layer_norm.bias": torch.zeros(c),
               "encoder.upsample.projection.weight": r(s * c, c), "encoder.upsample.projection.bias": torch.zeros(s * c)})
    for i in range(cfg.num_hidden_layers):
        p = f"encoder.layers.{i}."
        for n in ("q", "k", "v", "out"):
            sd[p + f"attention.{n}_proj.weight"], sd[p + f"attention.{n}_proj.bias"] = r(c, c), torch.zeros(c)
        sd[p + "layer_norm.weight"], sd[p + "layer_norm.bias"] = torch.ones(c), torch.zeros(c)
        sd[p + "feed_forward.intermediate_dense.weight"], sd[p + "feed_forward.intermediate_dense.bias"] = r(cfg.intermediate_size, c), torch.zeros(cfg.intermediate_size)
        sd[p + "feed_forward.output_dense.weight"], sd[p + "feed_forward.output_dense.bias"] = r(c, cfg.intermediate_size), torch.zeros(c)
        sd[p + "final_layer_norm.weight"], sd[p + "final_layer_norm.bias"] = torch.ones(c), torch.zeros(c)
    return sd


def squeeze_floor(b, t, c, groups, k, s):
    """(flop, bytes) of the matrix-core launch pair computed from shapes: the conv's multiply-adds at the checkpoint's width; one f32 read of x (pad
    kernel; the pool's second read is counted as cache hits), the bf16 padded copy written and read back, one f32 write of y."""
    t2, cg = t // s, c // groups
    prow = -(-(t + k) // s) * s
    flop = 2.0 * b * t2 * c * cg * k
    x_read, copy, y_write = b * t * c * 4, b * prow * groups * 32 * 2, b * t2 * c * 4
    return flop, (x_read, copy, y_write)


def time_launches(a, t=999, reps=20):
    """Per-call device time (events, best of three alternating blocks of `reps`) of the squeeze in both precisions and of the upsampler."""
    from thunder_speech_amd import _lib
    from thunder_speech_amd.huggingface.sew import pack_squeeze_taps, squeeze_on_matrix_cores
    L = _lib.lib()
    b, c, groups, k, s = a.batch, a.hidden, a.groups, a.taps, a.squeeze
    if not squeeze_on_matrix_cores(c // groups, k, s):
        raise SystemExit("bench_sew: this geometry has no matrix-core squeeze kernel; there is nothing to compare")
    t2 = t // s
    g = torch.Generator().manual_seed(4)
    st = torch.cuda.current_stream().cuda_stream
    x = torch.randn(b, t, c, generator=g).cuda()
    w = (torch.randn(c, c // groups, k, generator=g) * (c // groups * k) ** -0.5).cuda()
    bias = (0.1 * torch.randn(c, generator=g)).cuda()
    w16, w32 = pack_squeeze_taps(w, groups, True), pack_squeeze_taps(w, groups, False)
    ws = torch.empty(L.ts_sew_squeeze_workspace_bytes(b, t, c, k, s, 1), dtype=torch.uint8, device="cuda")
    y16, y32 = torch.empty(b, t2, c, device="cuda"), torch.empty(b, t2, c, device="cuda")
    h16 = torch.randn(b * t2, c, generator=g).to(torch.bfloat16).cuda()
    wu = (0.05 * torch.randn(s * c, c, generator=g)).to(torch.bfloat16).cuda()
    frag = torch.empty_like(wu)
    _lib.check(L.ts_gemm_nt_pack_w(wu.data_ptr(), c, s * c, c, frag.data_ptr(), st), "ts_gemm_nt_pack_w")
    bu = torch.zeros(s * c, device="cuda")
    up, out = torch.empty(b, t2, s * c, device="cuda"), torch.empty(b, t, c, device="cuda")
    calls = {
        "ts_sew_squeeze_fwd precision 1 (matrix cores)": lambda: L.ts_sew_squeeze_fwd(x.data_ptr(), b, t, c, w16.data_ptr(), bias.data_ptr(), k, groups, s, 1,
                                                                                      y16.data_ptr(), ws.data_ptr(), st),
        "ts_sew_squeeze_fwd precision 0 (f32 GEMM path)": lambda: L.ts_sew_squeeze_fwd(x.data_ptr(), b, t, c, w32.data_ptr(), bias.data_ptr(), k, groups, s, 0,
                                                                                       y32.data_ptr(), ws.data_ptr(), st),
        f"upsampler GEMM {c} -> {s * c}, GELU epilogue": lambda: L.ts_w2v_linear_fwd(h16.data_ptr(), c, wu.data_ptr(), bu.data_ptr(), None, s * c, up.data_ptr(),
                                                                                   s * c, None, b * t2, s * c, c, 1, 1, frag.data_ptr(), st),
    }
    if s * t2 != t:
        calls["ts_sew_unsqueeze_rows"] = lambda: L.ts_sew_unsqueeze_rows(up.data_ptr(), b, t2, t, c, s, out.data_ptr(), st)
    best = {name: float("inf") for name in calls}
    for _ in range(3):
        for name, f in calls.items():
            _lib.check(f(), name)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                f()
            e1.record(); torch.cuda.synchronize()
            best[name] = min(best[name], e0.elapsed_time(e1) / reps * 1e3)
    diff = float((y16 - y32).abs().max()) / float(y32.abs().max())
    return best, diff


def train_model(sew: bool, a, seed=0):
    """The SEW geometry of the arguments, or the wav2vec2-base geometry (768 / 12 heads / 12 layers / 3072, group-norm extractor, post-LN), as a
    transformers module: random weights, dropouts 0.1 and mask_time_prob 0.05 as in fine-tuning recipes."""
    import transformers
    kw = dict(hidden_dropout=0.1, attention_dropout=0.1, activation_dropout=0.1, feat_proj_dropout=0.1, layerdrop=0.0, mask_time_prob=0.05,
              mask_feature_prob=0.0, vocab_size=32)
    torch.manual_seed(seed)
    if not sew:
        return transformers.Wav2Vec2Model(transformers.Wav2Vec2Config(**kw, hidden_size=768, num_hidden_layers=12, num_attention_heads=12,
                                                                      intermediate_size=3072))
    return transformers.SEWModel(transformers.SEWConfig(**kw, hidden_size=a.hidden, num_hidden_layers=a.layers, num_attention_heads=a.heads,
                                                        intermediate_size=a.ffn, num_conv_pos_embeddings=a.taps, num_conv_pos_embedding_groups=a.groups,
                                                        squeeze_factor=a.squeeze, conv_dim=SEW_CONV_DIM, conv_stride=SEW_CONV_STRIDE,
                                                        conv_kernel=SEW_CONV_KERNEL))


def train_floors(b, t, c, groups, k, s):
    """{launch: (flop, bytes it must move)} from shapes.  Each conv product is the forward's 2 B T2 C cg k; a padded bf16 copy counts written and read
    back once (the re-reads of the weight gradient's workgroups are cache traffic, not counted)."""
    t2, cg, cp = t // s, c // groups, groups * 32
    prow, nt = -(-(t + k) // s) * s, -(-k // s)
    flop = 2.0 * b * t2 * c * cg * k
    x32, y32 = b * t * c * 4, b * t2 * c * 4
    fwd = x32 + 2 * b * prow * cp * 2 + y32
    return {"ts_sew_squeeze_fwd": (flop, fwd),
            "ts_sew_squeeze_train_fwd": (flop, fwd + y32),
            "ts_sew_squeeze_dgrad": (flop, 2 * y32 + 2 * b * (t2 + nt) * cp * 2 + x32),
            "ts_sew_squeeze_wgrad": (flop, y32 + x32 + 2 * b * (prow + t2) * cp * 2 + k * groups * cg * cg * 4)}


def time_train_launches(a, b=16, t=999, reps=20):
    """{launch: us per call}: device events, best of three alternating blocks of `reps` after one warm-up call each, all on the same tensors."""
    from thunder_speech_amd import _lib
    from thunder_speech_amd.huggingface.sew import pack_squeeze_taps
    from thunder_speech_amd.huggingface.sew_train import pack_squeeze_dgrad_taps, squeeze_trains
    L = _lib.lib()
    c, groups, k, s = a.hidden, a.groups, a.taps, a.squeeze
    cg = c // groups
    if not squeeze_trains(cg, k, s):
        raise SystemExit("bench_sew: this geometry does not train (24 or 32 channels per group do)")
    t2 = t // s
    g = torch.Generator().manual_seed(4)
    st = torch.cuda.current_stream().cuda_stream
    x = torch.randn(b, t, c, generator=g).cuda()
    w = (torch.randn(c, cg, k, generator=g) * (cg * k) ** -0.5).cuda()
    bias = (0.1 * torch.randn(c, generator=g)).cuda()
    dz, dy = torch.randn(b, t2, c, generator=g).cuda(), torch.randn(b, t2, c, generator=g).cuda()
    w16 = pack_squeeze_taps(w, groups, True)
    wd16 = pack_squeeze_dgrad_taps(w.view(groups, cg, cg, k).permute(3, 0, 1, 2).contiguous(), s)
    ws = lambda n: torch.empty(n, dtype=torch.uint8, device="cuda")
    ws_f, ws_d, ws_w = ws(L.ts_sew_squeeze_workspace_bytes(b, t, c, k, s, 1)), ws(L.ts_sew_squeeze_dgrad_workspace_bytes(b, t, c, k, s)), \
        ws(L.ts_sew_squeeze_wgrad_workspace_bytes(b, t, c, k, s))
    y, y2, z = (torch.empty(b, t2, c, device="cuda") for _ in range(3))
    dx, dw = torch.empty(b, t, c, device="cuda"), torch.empty(k, groups, cg, cg, device="cuda")
    calls = {
        "ts_sew_squeeze_fwd": lambda: L.ts_sew_squeeze_fwd(x.data_ptr(), b, t, c, w16.data_ptr(), bias.data_ptr(), k, groups, s, 1, y.data_ptr(),
                                                           ws_f.data_ptr(), st),
        "ts_sew_squeeze_train_fwd": lambda: L.ts_sew_squeeze_train_fwd(x.data_ptr(), b, t, c, w16.data_ptr(), bias.data_ptr(), k, groups, s, y2.data_ptr(),
                                                                       z.data_ptr(), ws_f.data_ptr(), st),
        "ts_sew_squeeze_dgrad": lambda: L.ts_sew_squeeze_dgrad(dz.data_ptr(), dy.data_ptr(), b, t, c, wd16.data_ptr(), k, groups, s, dx.data_ptr(),
                                                               ws_d.data_ptr(), st),
        "ts_sew_squeeze_wgrad": lambda: L.ts_sew_squeeze_wgrad(dz.data_ptr(), x.data_ptr(), b, t, c, k, groups, s, dw.data_ptr(), ws_w.data_ptr(), st),
    }
    best = {name: float("inf") for name in calls}
    for _ in range(3):
        for name, f in calls.items():
            _lib.check(f(), name)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                f()
            e1.record(); torch.cuda.synchronize()
            best[name] = min(best[name], e0.elapsed_time(e1) / reps * 1e3)
    assert torch.equal(y, y2), "ts_sew_squeeze_train_fwd: y differs from ts_sew_squeeze_fwd's"
    return best


def main_train(a):
    from tools.bench_wavlm import time_train
    rows = []
    for name, pick in (("wav2vec2-base geometry (768 / 12 heads / 12 layers / 3072)", False),
                       (f"sew ({a.hidden} / {a.heads} heads / {a.layers} layers / {a.ffn}, {a.taps} taps in {a.groups} groups, squeeze {a.squeeze})", True)):
        model = train_model(pick, a)
        params = sum(p.numel() for p in model.parameters() if p.requires_grad)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        ms = time_train(name, model, a)
        rows.append((name, ms, torch.cuda.max_memory_allocated() / 2 ** 30, params))
        del model
        torch.cuda.empty_cache()
    b, t = 16, 999
    launches = time_train_launches(a, b, t)
    floors = train_floors(b, t, a.hidden, a.groups, a.taps, a.squeeze)
    frames = (16000 * a.seconds - 400) // 320 + 1
    lines = [f"fine-tuning step, train_precision=\"bf16\": {a.batch} x {a.seconds} s (one clip 3/4 long; t = {frames} frames), dropouts 0.1, mask_time_prob 0.05; "
             f"{a.steps} timed steps after 2 warm-up steps, host clock around a device synchronise.  The SEW geometry is sew-mid as recalled, not verified "
             "against the published checkpoint.", "",
             "| model | trained parameters | ms/step | vs wav2vec2-base geometry | peak allocated GiB |", "|---|---:|---:|---:|---:|"]
    for name, ms, gib, params in rows:
        lines.append(f"| {name} | {params / 1e6:.0f} M | {ms:.1f} | {ms / rows[0][1]:.3f} | {gib:.2f} |")
    fwd = launches["ts_sew_squeeze_fwd"]
    lines += ["", f"the squeeze's launches, {b} clips x t = {t} x {a.hidden} channels, {a.taps} taps in {a.groups} groups, stride {a.squeeze} (device events, best "
              "of 3 alternating blocks of 20 calls after a warm-up call; every call is its padded bf16 copies plus its kernel; same tensors for all four); "
              "floor = the larger of FLOPs / 2.5 PFLOP/s and bytes / 8 TB/s:", "",
              "| call | us per call | vs ts_sew_squeeze_fwd | GFLOP | MB it must move | floor us | floor / measured |", "|---|---:|---:|---:|---:|---:|---:|"]
    for name, us in launches.items():
        flop, nbytes = floors[name]
        floor = max(flop / PEAK_BF16, nbytes / PEAK_HBM) * 1e6
        lines.append(f"| {name} | {us:.1f} | {us / fwd:.2f} | {flop / 1e9:.1f} | {nbytes / 1e6:.1f} | {floor:.1f} | {floor / us:.2f} |")
    over = [name for name in ("ts_sew_squeeze_dgrad", "ts_sew_squeeze_wgrad") if launches[name] > 3 * fwd]
    lines += ["", ("Over 3x the forward call on the same shape: " + ", ".join(over) + " -- what bounds each is named below." if over else
                   "Neither new launch takes more than 3x the forward call on the same shape.")]
    return lines


def main():
    ap = argparse.ArgumentParser(description="SEW forward on the HIP path next to wav2vec2-base geometry.  The geometry defaults are sew-mid as "
                                             "recalled, NOT verified against the published checkpoint.")
    ap.add_argument("--batch", type=int, default=None, help="default 16 (inference), 8 (--train)")
    ap.add_argument("--seconds", type=int, default=None, help="default 20 (inference), 10 (--train)")
    ap.add_argument("--train", action="store_true", help="mixed-precision fine-tuning steps and the launches of csrc/sew_train.hip instead of inference")
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--ffn", type=int, default=2048)
    ap.add_argument("--taps", type=int, default=128)
    ap.add_argument("--groups", type=int, default=16)
    ap.add_argument("--squeeze", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the tables (markdown) to this file")
    a = ap.parse_args()
    a.batch = a.batch or (8 if a.train else 16)
    a.seconds = a.seconds or (10 if a.train else 20)
    if not torch.cuda.is_available():
        raise SystemExit("bench_sew: needs an MI355X")
    if a.train:
        text = "\n".join(main_train(a))
        print(text)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text + "\n")
        return
    from thunder_speech_amd.huggingface.encoder import Wav2Vec2Plan
    from thunder_speech_amd.huggingface.sew import SEWPlan
    base_cfg = config(True, 12)
    cfg = sew_config(a)
    rows, frames = [], {}
    for name, make in (("wav2vec2-base geometry (768 / 12 heads / 12 layers / 3072)", lambda: Wav2Vec2Plan(base_cfg, random_state(base_cfg), "cuda", precision="bf16")),
                       (f"sew ({a.hidden} / {a.heads} heads / {a.layers} layers / {a.ffn}, squeeze {a.squeeze})",
                        lambda: SEWPlan(cfg, sew_random_state(cfg), "cuda", precision="bf16"))):
        plan = make()
        r, frames[name] = time_model(name, plan, a)
        del plan
        torch.cuda.empty_cache()
        rows.append((name, r))
    launches, diff = time_launches(a)
    flop, (x_read, copy, y_write) = squeeze_floor(a.batch, 999, a.hidden, a.groups, a.taps, a.squeeze)
    nbytes = x_read + 2 * copy + y_write
    floor_us = max(flop / PEAK_BF16, nbytes / PEAK_HBM) * 1e6
    base = rows[0][1]
    lines = [f"Measured: {a.batch} x {a.seconds} s, bf16, frames out {', '.join(str(v) for v in frames.values())}; {a.steps} timed steps per mode after warm-up. "
             "The SEW geometry is sew-mid as recalled, not verified against the published checkpoint.", "",
             "| model | eager ms/step | graphed ms/step | graphed vs wav2vec2-base geometry |", "|---|---:|---:|---:|"]
    for name, r in rows:
        lines.append(f"| {name} | {r['eager']:.1f} | {r['graphed']:.1f} | {r['graphed'] / base['graphed']:.3f} |")
    m16 = launches["ts_sew_squeeze_fwd precision 1 (matrix cores)"]
    m32 = launches["ts_sew_squeeze_fwd precision 0 (f32 GEMM path)"]
    lines += ["", f"launches, {a.batch} clips x t = 999 x {a.hidden} channels (device events, best of 3 alternating blocks of 20; each squeeze call is the padded copy "
              "plus its kernels):", "", "| call | us per call |", "|---|---:|"]
    lines += [f"| {name} | {us:.1f} |" for name, us in launches.items()]
    lines += ["", f"Squeeze A/B in this run: matrix cores {m16:.1f} us, f32 path {m32:.1f} us: {m32 / m16:.1f}x"
              + ("." if m16 < m32 else " -- the matrix-core kernel is NOT faster.")
              + f"  The two results differ by {diff:.2e} of max |y| (bf16 operands against f32).", "",
              f"Computed floor of the matrix-core call at t = 999: {flop / 1e9:.1f} GFLOP -> {flop / PEAK_BF16 * 1e6:.1f} us at the 2.5 PFLOP/s bf16 spec peak; bytes: "
              f"x read {x_read / 1e6:.1f} MB (f32) + padded bf16 copy {copy / 1e6:.1f} MB written and read back + y written {y_write / 1e6:.1f} MB (f32) = "
              f"{nbytes / 1e6:.1f} MB -> {nbytes / PEAK_HBM * 1e6:.1f} us at the 8.0 TB/s spec peak ({nbytes / COPY_HBM * 1e6:.1f} us at the 6.29 TB/s a float4 copy "
              f"reaches).  The larger of the two bounds, {floor_us:.1f} us, is {floor_us / m16 * 100:.0f} % of the measured {m16:.1f} us "
              f"({flop / m16 / 1e6:.0f} TFLOP/s achieved over the whole call)."]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
