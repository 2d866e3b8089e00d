"""Mixed-precision fine-tuning steps (train_precision="bf16": training forward, backward of a probe loss, AdamW) of the families huggingface/train.py
trains besides wav2vec2 and WavLM, random weights, 8 x 10 s, in ONE process with alternating blocks:
  hubert-large            1024 hidden, 24 layers, pre-LN, layer-norm convs, weight-normalised positional conv (k 128, 16 groups)
  data2vec-audio-large    1024 hidden, 24 layers, post-LN, positional stack 5 x k 19 x 16 groups (64 channels per group: the matrix-core conv)
  data2vec-audio-base     768 hidden, 12 layers, the same stack at 48 channels per group (the f32-GEMM conv branch of PosConvStackLayer)
  wav2vec2-large post-LN  the yardstick: the same encoder layers as data2vec-audio-large, only the positional embedding differs
-- ms per step and peak allocated memory per geometry, the positional stack's share of the data2vec steps (its five nodes, forward + backward, timed
alone at the step's shape) -- and the per-call times of the node's launches at that shape (rows = batch x t = 3 992) for C = 1024 and C = 768:
  ts_posconv_stack_norm_gelu_fwd   next to its HBM floor (read z, write a: 8 B per element) and to ts_w2v_layernorm_fwd(xbias, act = 1)
  ts_posconv_stack_norm_gelu_bwd   next to its HBM floor (read da and z, write dz: 12 B per element) and to the three-pass composition it replaces:
                                   ts_w2v_gelu_bwd + ts_w2v_layernorm_bwd_set with a unit gamma (+ ts_w2v_colsum for the bias gradient)
  ts_posconv_stack_conv            forward and data gradient next to ts_w2v_posconv_train at the same t, k, groups (C = 1024 only: 64 per group)
Device events, 3 alternating blocks per call, the best block (tools/bench_mms.py's conventions).
python tools/bench_family_finetune.py [--batch 8] [--seconds 10] [--steps 8] [--layers N] [--out FILE.md]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tools.bench_mms import HBM_PEAK, _best_of_blocks, graph_nodes

RECIPE = dict(hidden_dropout=0.1, attention_dropout=0.1, activation_dropout=0.1, feat_proj_dropout=0.1, layerdrop=0.0, mask_time_prob=0.05,
              mask_feature_prob=0.0, vocab_size=32)
LARGE = dict(hidden_size=1024, num_attention_heads=16, intermediate_size=4096)
BASE = dict(hidden_size=768, num_attention_heads=12, intermediate_size=3072)
GEOMETRIES = {
    "hubert-large": ("Hubert", 24, dict(LARGE, feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True, feat_proj_layer_norm=True)),
    "data2vec-audio-large": ("Data2VecAudio", 24, dict(LARGE, num_conv_pos_embeddings=5, conv_pos_kernel_size=19, num_conv_pos_embedding_groups=16)),
    "data2vec-audio-base": ("Data2VecAudio", 12, dict(BASE, num_conv_pos_embeddings=5, conv_pos_kernel_size=19, num_conv_pos_embedding_groups=16)),
    "wav2vec2-large post-LN": ("Wav2Vec2", 24, dict(LARGE, feat_extract_norm="group", do_stable_layer_norm=False, conv_bias=False)),
}


def build_model(name, layers=None, seed=0):
    import transformers
    cls, n, kw = GEOMETRIES[name]
    torch.manual_seed(seed)
    m = getattr(transformers, cls + "Model")(getattr(transformers, cls + "Config")(num_hidden_layers=layers or n, **kw, **RECIPE))
    with torch.no_grad():          # transformers leaves every conv bias at zero: a zero-padded row of the stack would have variance exactly 0
        for pname, p in m.named_parameters():
            if p.dim() == 1 and "bias" in pname:
                p.add_(0.05 * torch.randn_like(p))
    return m


def time_steps(a, rounds=2, n_inputs=3):
    """{geometry: [ms / step of each block]}, {geometry: peak bytes}, {geometry: node names}, t; one process, 2 warm-up steps per geometry, then
    `rounds` alternating blocks of steps / rounds timed steps each between device events; the inputs rotate over `n_inputs` seeded batches."""
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    g = torch.Generator().manual_seed(0)
    xs = [(0.1 * torch.randn(a.batch, 16000 * a.seconds, generator=g)).cuda() for _ in range(n_inputs)]
    lengths = torch.full((a.batch,), 16000 * a.seconds, dtype=torch.int64, device="cuda")
    lengths[-1] = 16000 * a.seconds * 3 // 4                                  # one ragged clip
    runs = {}
    for name in GEOMETRIES:
        adapt = HuggingFaceEncoderAdapt(build_model(name, a.layers), mask_input=True, train_precision="bf16").cuda().train()
        runs[name] = dict(adapt=adapt, opt=torch.optim.AdamW([p for p in adapt.parameters() if p.requires_grad], lr=1e-5), probe=None, i=0, nodes=None)

    def step(r, walk=False):
        r["opt"].zero_grad(set_to_none=True)
        feats, _ = r["adapt"](xs[r["i"] % n_inputs], lengths)
        r["i"] += 1
        if r["probe"] is None:
            r["probe"], r["t"] = torch.randn(feats.shape, generator=g).cuda(), feats.shape[-1]
        if walk:
            r["nodes"] = graph_nodes(feats.grad_fn)
        (feats * r["probe"]).mean().backward()
        r["opt"].step()

    for r in runs.values():
        for i in range(2):
            step(r, walk=i == 0)
    torch.cuda.synchronize()
    per = max(1, (a.steps + rounds - 1) // rounds)
    blocks, peak = {k: [] for k in runs}, {k: 0 for k in runs}
    for _ in range(rounds):
        for name, r in runs.items():
            torch.cuda.reset_peak_memory_stats()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(per + 1)]
            ev[0].record()
            for i in range(per):
                step(r)
                ev[i + 1].record()
            torch.cuda.synchronize()
            ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(per)]
            print(f"  block of {name}: " + " ".join(f"{x:.1f}" for x in ms) + " ms", flush=True)
            blocks[name].append(sum(ms) / per)
            peak[name] = max(peak[name], torch.cuda.max_memory_allocated())
    t = next(iter(runs.values()))["t"]
    nodes = {k: r["nodes"] for k, r in runs.items()}
    runs.clear()
    torch.cuda.empty_cache()
    return blocks, peak, nodes, t, per * rounds


def time_stack(a, t, c, groups=16, k=19, n=5, reps=10):
    """ms of the positional stack alone -- n PosConvStackLayer nodes, forward + backward, mixed mode -- at [batch, t, c]: the best of three blocks."""
    from thunder_speech_amd.huggingface import train as T
    g = torch.Generator().manual_seed(5)
    cg = c // groups
    x = torch.randn(a.batch, t, c, generator=g).cuda().requires_grad_(True)
    ws = [(torch.randn(k, groups, cg, cg, generator=g) * (cg * k) ** -0.5).cuda().requires_grad_(True) for _ in range(n)]
    bs = [(0.05 * torch.randn(c, generator=g)).cuda().requires_grad_(True) for _ in range(n)]
    dy = torch.randn(a.batch, t, c, generator=g).cuda()

    def once():
        p = x
        for w, b in zip(ws, bs):
            p = T.PosConvStackLayer.apply(p, w, b)
        p.backward(dy)

    best = float("inf")
    with T.mixed_precision(True):
        once()
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                once()
            e1.record(); torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1) / reps)
    return best


def row_kernel_calls(rows, c):
    """{name: call}, {name: HBM floor in us} of the node's row launches and of what they replace, f32 [rows][c]."""
    from thunder_speech_amd import _lib
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(c)
    z, da = (2.0 * torch.randn(rows, c, generator=g) + 3.0).cuda(), torch.randn(rows, c, generator=g).cuda()
    bias, ones, zeros = (0.05 * torch.randn(c, generator=g)).cuda(), torch.ones(c).cuda(), torch.zeros(c).cuda()
    out, dn, dz = (torch.empty(rows, c, device="cuda") for _ in range(3))
    zb = z + bias                                               # the composition's LayerNorm backward takes no bias: it reads a materialised z + bias
    n = torch.nn.functional.layer_norm(zb, (c,), eps=1e-5)
    db, dg, dbeta = (torch.empty(c, device="cuda") for _ in range(3))
    ws = torch.empty(L.ts_posconv_stack_norm_gelu_bwd_workspace(rows, c), dtype=torch.uint8, device="cuda")
    ws_ln = torch.empty(L.ts_w2v_layernorm_bwd_workspace(rows, c), dtype=torch.uint8, device="cuda")
    e = rows * c

    def composition():
        st = L.ts_w2v_gelu_bwd(n.data_ptr(), None, c, da.data_ptr(), dn.data_ptr(), e, s)
        return st or L.ts_w2v_layernorm_bwd_set(zb.data_ptr(), None, ones.data_ptr(), dn.data_ptr(), 1e-5, rows, c, dz.data_ptr(), dg.data_ptr(), dbeta.data_ptr(),
                                                ws_ln.data_ptr(), s)

    def composition_colsum():
        db.zero_()
        return composition() or L.ts_w2v_colsum(dz.data_ptr(), rows, c, c, db.data_ptr(), s)

    calls = {
        f"ts_posconv_stack_norm_gelu_fwd, C = {c}": lambda: L.ts_posconv_stack_norm_gelu_fwd(z.data_ptr(), bias.data_ptr(), 1e-5, rows, c, out.data_ptr(), s),
        f"ts_w2v_layernorm_fwd(xbias, act = 1), C = {c}": lambda: L.ts_w2v_layernorm_fwd(z.data_ptr(), None, bias.data_ptr(), ones.data_ptr(), zeros.data_ptr(), 1e-5,
                                                                                         rows, c, 1, out.data_ptr(), None, s),
        f"ts_posconv_stack_norm_gelu_bwd (dz + dbias), C = {c}": lambda: L.ts_posconv_stack_norm_gelu_bwd(z.data_ptr(), bias.data_ptr(), da.data_ptr(), 1e-5, rows, c,
                                                                                                         dz.data_ptr(), db.data_ptr(), ws.data_ptr(), s),
        f"ts_w2v_gelu_bwd + ts_w2v_layernorm_bwd_set (unit gamma), C = {c}": composition,
        f"the same + zero fill + ts_w2v_colsum (dbias), C = {c}": composition_colsum,
    }
    floors = {k: (8 if "_fwd" in k else 12) * e / HBM_PEAK * 1e6 for k in calls}          # the forward calls are the two whose names hold "_fwd"
    return calls, floors


def conv_calls(a, t, c=1024, groups=16, k=19):
    from thunder_speech_amd import _lib
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(7)
    b = a.batch
    x, res = torch.randn(b, t, c, generator=g).cuda(), torch.randn(b, t, c, generator=g).cuda()
    w16 = (torch.randn(k, groups, 64, 64, generator=g) * (64 * k) ** -0.5).to(torch.bfloat16).cuda()
    bias = torch.zeros(c).cuda()
    y, z = torch.empty_like(x), torch.empty_like(x)
    ws = torch.empty(L.ts_posconv_stack_conv_workspace(b, t, c, k), dtype=torch.uint8, device="cuda")
    return {
        "ts_posconv_stack_conv forward (raw epilogue)": lambda: L.ts_posconv_stack_conv(x.data_ptr(), b, t, c, w16.data_ptr(), k, groups, 0, z.data_ptr(), ws.data_ptr(), s),
        "ts_w2v_posconv_train forward (bias + GELU + residual, z kept)": lambda: L.ts_w2v_posconv_train(x.data_ptr(), x.data_ptr(), b, t, c, w16.data_ptr(), bias.data_ptr(), k,
                                                                                                        groups, 0, y.data_ptr(), z.data_ptr(), ws.data_ptr(), s),
        "ts_posconv_stack_conv data gradient (raw epilogue)": lambda: L.ts_posconv_stack_conv(x.data_ptr(), b, t, c, w16.data_ptr(), k, groups, 1, z.data_ptr(), ws.data_ptr(), s),
        "ts_w2v_posconv_train data gradient (+ residual)": lambda: L.ts_w2v_posconv_train(x.data_ptr(), res.data_ptr(), b, t, c, w16.data_ptr(), None, k, groups, 1, y.data_ptr(),
                                                                                          None, ws.data_ptr(), s),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seconds", type=int, default=10)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--layers", type=int, default=None, help="encoder layers of every geometry (default: 24 / 24 / 12 / 24)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_family_finetune: no GPU (nothing is measured on the CPU)")
    lines = [f"# Fine-tuning steps of HuBERT and data2vec-audio geometries ({torch.cuda.get_device_name(0)})", "",
             f"`python tools/bench_family_finetune.py --batch {a.batch} --seconds {a.seconds} --steps {a.steps}"
             + (f" --layers {a.layers}" if a.layers else "") + "`: random weights, train_precision=\"bf16\", AdamW, dropouts 0.1, mask_time_prob 0.05, one ragged clip;",
             "one process, alternating blocks between device events.", ""]
    blocks, peak, nodes, t, timed = time_steps(a)
    rows = a.batch * t
    best = {k: min(v) for k, v in blocks.items()}
    stack = {"data2vec-audio-large": time_stack(a, t, 1024), "data2vec-audio-base": time_stack(a, t, 768)}
    lines += [f"## The step ({a.batch} x {a.seconds} s, t = {t} frames, {timed} timed steps per geometry)", "",
              "| geometry | ms / step, best block (all blocks) | peak allocated GiB | positional stack alone, fwd + bwd, ms (share of the step) |", "|---|---|---|---|"]
    for k in blocks:
        share = f"{stack[k]:.2f} ({100 * stack[k] / best[k]:.1f} %)" if k in stack else "--"
        lines.append(f"| {k} | {best[k]:.1f} ({', '.join(f'{x:.1f}' for x in blocks[k])}) | {peak[k] / 2 ** 30:.2f} | {share} |")
    lines += ["", "Autograd nodes of the data2vec-audio-large graph: " + ", ".join(f"{n} x {c}" for n, c in sorted(nodes["data2vec-audio-large"].items())
                                                                               if n.endswith("Backward") and not n[0].islower()), ""]
    lines += [f"## The node's row launches at rows = {rows}", "", f"HBM floor at {HBM_PEAK / 1e12:.1f} TB/s: forward 8 B, backward 12 B per element.", "",
              "| call | us | HBM floor us |", "|---|---|---|"]
    slower = []
    for c in (1024, 768):
        calls, floors = row_kernel_calls(rows, c)
        us = _best_of_blocks(calls, 50)
        for k in calls:
            lines.append(f"| {k} | {us[k]:.1f} | {floors[k]:.1f} |")
        fused, comp = us[f"ts_posconv_stack_norm_gelu_bwd (dz + dbias), C = {c}"], us[f"ts_w2v_gelu_bwd + ts_w2v_layernorm_bwd_set (unit gamma), C = {c}"]
        if fused > comp:
            slower.append(f"C = {c}: the fused backward row kernel ({fused:.1f} us) is SLOWER than the composition ({comp:.1f} us).")
    lines += [""] + (slower or ["The fused backward row kernel is faster than the composition at both widths."]) + [""]
    us = _best_of_blocks(conv_calls(a, t), 50)
    lines += [f"## The matrix-core conv at {a.batch} x {t} x 1024, k 19, 16 groups", "", "| call (pad + conv launch) | us |", "|---|---|"]
    lines += [f"| {k} | {v:.1f} |" for k, v in us.items()]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
