"""precision="mxfp8" next to precision="bf16" on one MI355X, same process (random weights of the named geometries: nothing here speaks about a
trained checkpoint's transcripts):
  * forward steps at the C5 geometry (wav2vec2-large, 16 x 20 s) and the XLS-R 1B geometry (hidden 1280, 48 layers, head_dim 80, pre-LN), eager and
    graphed, in the order bf16, mxfp8, bf16 again -- the two bf16 timings show the run's spread;
  * the four layer products per call: ts_mx_gemm_nt with the epilogue the plan uses against ts_gemm_nt_bf16_packed with the matching one, TFLOP/s;
  * ts_mx_quantize_rows and ts_mx_layernorm_fwd next to their HBM floors and to ts_w2v_layernorm_fwd;
  * the deviation of both modes from the "fp32" plan on the same (smaller) batch: rms and max in units of the output's rms.
python tools/bench_mxfp8.py [--batch 16] [--seconds 20] [--steps 50] [--layers-c5 24] [--layers-xlsr 48] [--geometry all|c5|xlsr] [--out FILE.md]
Exit status 1 when the mxfp8 step at the C5 geometry is not faster than bf16 by more than the gap between the two bf16 timings, or a product is
not faster per call than ts_gemm_nt_bf16_packed (the middle one of three blocks each): the table says where the time goes."""
import argparse
import os
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tools.bench_c5 import config, random_state
from tools.bench_wavlm import layer_norm_variant

HBM_PEAK = 8.0e12          # bytes / s, MI355X data sheet


def geometries(a):
    c5 = config(False, a.layers_c5)
    x1 = config(False, a.layers_xlsr)
    x1 = SimpleNamespace(**{**vars(x1), "hidden_size": 1280, "intermediate_size": 5120, "num_attention_heads": 16})
    x1, x1_sd = layer_norm_variant(x1, random_state(x1), False)
    return {"C5 (wav2vec2-large)": (c5, random_state(c5)), "XLS-R 1B": (x1, x1_sd)}


def time_steps(cfg, sd, a):
    """-> ({(precision label, mode): ms / step}, frames): plans of both modes alive together, timed in the order bf16, mxfp8, bf16."""
    from thunder_speech_amd.huggingface.encoder import Wav2Vec2Plan
    from thunder_speech_amd.huggingface.transform import Wav2Vec2Preprocess
    pre = Wav2Vec2Preprocess()
    x = (0.1 * torch.randn(a.batch, 16000 * a.seconds, generator=torch.Generator().manual_seed(0))).cuda()
    lengths = torch.full((a.batch,), 16000 * a.seconds, dtype=torch.int32, device="cuda")
    res, runs = {}, {}
    with torch.no_grad():
        for precision in ("bf16", "mxfp8"):
            plan = Wav2Vec2Plan(cfg, sd, "cuda", precision=precision)

            def step(plan=plan):
                xn, _ = pre(x, lengths)
                return plan.forward(xn, None)
            out = step(); out = step(); torch.cuda.synchronize()
            assert torch.isfinite(out).all(), precision
            graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
            with torch.cuda.stream(side):
                with torch.cuda.graph(graph, stream=side):
                    gout = step()
            graph.replay(); torch.cuda.synchronize()
            if not torch.equal(gout, out):
                print(f"{precision}: graph replay differs from the eager forward by {float((gout - out).abs().max()):.3g}")
            runs[precision] = {"eager": step, "graphed": graph.replay, "keep": (plan, graph, gout)}
        for label, precision in (("bf16 (first)", "bf16"), ("mxfp8", "mxfp8"), ("bf16 (second)", "bf16")):
            for mode in ("eager", "graphed"):
                run = runs[precision][mode]
                run(); run(); torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    run()
                torch.cuda.synchronize()
                res[(label, mode)] = (time.perf_counter() - t0) / a.steps * 1e3
    frames = out.shape[1]
    del runs
    torch.cuda.empty_cache()
    return res, frames


def deviation(cfg, sd, a, clips=2):
    """rms and max of (mode - fp32 plan) in units of the fp32 output's rms, on `clips` clips of the batch."""
    from thunder_speech_amd.huggingface.encoder import Wav2Vec2Plan
    from thunder_speech_amd.huggingface.transform import Wav2Vec2Preprocess
    pre = Wav2Vec2Preprocess()
    x = (0.1 * torch.randn(a.batch, 16000 * a.seconds, generator=torch.Generator().manual_seed(0)))[:clips].cuda()
    lengths = torch.full((clips,), 16000 * a.seconds, dtype=torch.int32, device="cuda")
    out = {}
    with torch.no_grad():
        xn, _ = pre(x, lengths)
        for precision in ("fp32", "bf16", "mxfp8"):
            plan = Wav2Vec2Plan(cfg, sd, "cuda", precision=precision)
            out[precision] = plan.forward(xn, None).double()
            del plan
            torch.cuda.empty_cache()
    unit = float(out["fp32"].pow(2).mean().sqrt())
    return {p: (float((out[p] - out["fp32"]).pow(2).mean().sqrt()) / unit, float((out[p] - out["fp32"]).abs().max()) / unit) for p in ("bf16", "mxfp8")}


def _blocks(calls, reps, blocks=3):
    """Per-launch device time (us) of each call, alternated in `blocks` blocks of `reps` launches between device events: {call: [us per block]}."""
    from thunder_speech_amd import _lib
    times = {k: [] for k in calls}
    for _ in range(blocks):
        for k, f in calls.items():
            _lib.check(f(), k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                f()
            e1.record(); torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / reps * 1e3)
    return times


def time_kernels(rows, c, ffn, reps=300):
    """-> (gemm rows [(name, n, k, [us mx per block], [us bf16 per block])], row-kernel rows [(name, [us per block], floor us)])"""
    from thunder_speech_amd import _lib
    L = _lib.lib()
    d = _lib.STAGED["mxfp8"].defines
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(1)
    u8 = lambda *shape: torch.empty(*shape, dtype=torch.uint8, device="cuda")
    gemms = []
    for name, n, k, ep in (("q / k / v", 3 * c, c, "bf16"), ("out_proj", c, c, "accum"), ("FFN in", ffn, c, "gelu"), ("FFN out", c, ffn, "accum")):
        x16 = torch.randn(rows, k, generator=g).to(torch.bfloat16).cuda()
        w32 = (torch.randn(n, k, generator=g) / k ** 0.5).cuda()
        w16 = w32.to(torch.bfloat16)
        bias = torch.zeros(n, device="cuda")
        wf16 = torch.empty_like(w16)
        _lib.check(L.ts_gemm_nt_pack_w(w16.data_ptr(), k, n, k, wf16.data_ptr(), s), "ts_gemm_nt_pack_w")
        xq, xs, wq, ws = u8(rows, k), u8(rows, k // 32), u8(n, k), u8(n, k // 32)
        _lib.check(L.ts_mx_quantize_rows(x16.data_ptr(), 1, k, rows, k, xq.data_ptr(), k, xs.data_ptr(), k // 32, s), "ts_mx_quantize_rows")
        _lib.check(L.ts_mx_quantize_rows(w32.data_ptr(), 0, k, n, k, wq.data_ptr(), k, ws.data_ptr(), k // 32, s), "ts_mx_quantize_rows")
        frag, sfrag = u8(n * k), u8(int(L.ts_mx_pack_w_scale_bytes(n, k)))
        _lib.check(L.ts_mx_pack_w(wq.data_ptr(), k, ws.data_ptr(), k // 32, n, k, frag.data_ptr(), sfrag.data_ptr(), s), "ts_mx_pack_w")
        y = torch.zeros(rows, n, device="cuda") if ep == "accum" else None
        y16 = torch.empty(rows, n, dtype=torch.bfloat16, device="cuda") if ep != "accum" else None
        yq, ys = (u8(rows, n), u8(rows, n // 32)) if ep == "gelu" else (None, None)
        p = lambda t: None if t is None else t.data_ptr()
        code = {"bf16": d["TS_MX_EP_BF16"], "accum": d["TS_MX_EP_ACCUM"], "gelu": d["TS_MX_EP_GELU_MX"]}[ep]
        calls = {
            "mx": lambda: L.ts_mx_gemm_nt(xq.data_ptr(), k, xs.data_ptr(), k // 32, frag.data_ptr(), sfrag.data_ptr(), bias.data_ptr(), code, p(y), n,
                                          p(y16) if ep == "bf16" else None, n, p(yq), n, p(ys), n // 32, rows, n, k, s),
            "bf16": lambda: L.ts_gemm_nt_bf16_packed(x16.data_ptr(), k, w16.data_ptr(), k, wf16.data_ptr(), bias.data_ptr(), p(y), n, p(y), n, p(y16), n,
                                                     rows, n, k, 1 if ep == "gelu" else 0, s),
        }
        t = _blocks(calls, reps)
        gemms.append((name, n, k, t["mx"], t["bf16"]))
        del x16, w32, w16, wf16, xq, xs, wq, ws, frag, sfrag, y, y16, yq, ys
    h = torch.randn(rows, c, generator=g).cuda()
    h16 = h.to(torch.bfloat16)
    ones, zeros = torch.ones(c).cuda(), torch.zeros(c).cuda()
    y16, q, sc = torch.empty(rows, c, dtype=torch.bfloat16, device="cuda"), u8(rows, c), u8(rows, c // 32)
    calls = {
        "ts_w2v_layernorm_fwd (bf16 result)": lambda: L.ts_w2v_layernorm_fwd(h.data_ptr(), None, None, ones.data_ptr(), zeros.data_ptr(), 1e-5, rows, c, 0,
                                                                             None, y16.data_ptr(), s),
        "ts_mx_layernorm_fwd (MX result)": lambda: L.ts_mx_layernorm_fwd(h.data_ptr(), None, None, ones.data_ptr(), zeros.data_ptr(), 1e-5, rows, c, None,
                                                                         q.data_ptr(), c, sc.data_ptr(), c // 32, s),
        "ts_mx_quantize_rows (bf16 rows)": lambda: L.ts_mx_quantize_rows(h16.data_ptr(), 1, c, rows, c, q.data_ptr(), c, sc.data_ptr(), c // 32, s),
    }
    floors = {"ts_w2v_layernorm_fwd (bf16 result)": rows * (4 * c + 2 * c) / HBM_PEAK * 1e6,
              "ts_mx_layernorm_fwd (MX result)": rows * (4 * c + c + c // 32) / HBM_PEAK * 1e6,
              "ts_mx_quantize_rows (bf16 rows)": rows * (2 * c + c + c // 32) / HBM_PEAK * 1e6}
    t = _blocks(calls, reps)
    return gemms, [(k, t[k], floors[k]) for k in calls]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seconds", type=int, default=20)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--layers-c5", type=int, default=24)
    ap.add_argument("--layers-xlsr", type=int, default=48)
    ap.add_argument("--geometry", choices=("all", "c5", "xlsr"), default="all")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines, ok = [], True
    say = lambda s="": (print(s, flush=True), lines.append(s))
    say(f"# precision=\"mxfp8\" against \"bf16\": {a.batch} x {a.seconds} s, random weights, {torch.cuda.get_device_name(0)}")
    for name, (cfg, sd) in geometries(a).items():
        if a.geometry != "all" and name.startswith("C5") != (a.geometry == "c5"):
            continue
        res, frames = time_steps(cfg, sd, a)
        rows, c, ffn, layers = a.batch * frames, cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers
        say(f"\n## {name}: hidden {c}, {layers} layers, {frames} frames per clip ({rows} rows)\n")
        say("| forward step | eager ms | graphed ms |")
        say("|---|---|---|")
        for label in ("bf16 (first)", "mxfp8", "bf16 (second)"):
            say(f"| {label} | {res[(label, 'eager')]:.2f} | {res[(label, 'graphed')]:.2f} |")
        b1, b2, mx = res[("bf16 (first)", "graphed")], res[("bf16 (second)", "graphed")], res[("mxfp8", "graphed")]
        faster = mx < min(b1, b2) - abs(b1 - b2)
        say(f"\ngraphed: mxfp8 {mx:.2f} ms against bf16 {min(b1, b2):.2f} ms (spread of the two bf16 timings {abs(b1 - b2):.2f} ms): "
            f"{'faster' if faster else 'NOT faster'} ({min(b1, b2) / mx:.3f} x)")
        if name.startswith("C5"):
            ok &= faster
        gemms, rowk = time_kernels(rows, c, ffn)
        say(f"\nper call: the best of three alternating blocks of 300 launches each (worst block in brackets); the operands of a call stay in the "
            f"last-level cache between launches, for both kernels alike\n")
        say("| product | n | k | ts_mx_gemm_nt us | TFLOP/s | ts_gemm_nt_bf16_packed us | TFLOP/s | mx / bf16 |")
        say("|---|---|---|---|---|---|---|---|")
        for gname, n, k, t_mx, t_bf in gemms:
            fl = 2.0 * rows * n * k
            say(f"| {gname} | {n} | {k} | {min(t_mx):.1f} ({max(t_mx):.1f}) | {fl / min(t_mx) * 1e-6:.0f} | {min(t_bf):.1f} ({max(t_bf):.1f}) | "
                f"{fl / min(t_bf) * 1e-6:.0f} | {min(t_mx) / min(t_bf):.3f} |")
            if name.startswith("C5"):
                ok &= sorted(t_mx)[1] < sorted(t_bf)[1]           # the middle block of each
        say("\n| row kernel (per call) | us | HBM floor us |")
        say("|---|---|---|")
        for k, t, fl in rowk:
            say(f"| {k} | {min(t):.1f} ({max(t):.1f}) | {fl:.1f} |")
        quant = min(dict((k, t) for k, t, _ in rowk)["ts_mx_quantize_rows (bf16 rows)"])
        say(f"\nthe quantiser of the attention context runs once per layer: {layers} x {quant:.1f} us = {layers * quant * 1e-3:.2f} ms, "
            f"{100 * layers * quant * 1e-3 / mx:.1f} % of the graphed mxfp8 step")
        dev = deviation(cfg, sd, a)
        say("\n| deviation from the fp32 plan (2 clips of the batch, units of the output's rms) | rms | max |")
        say("|---|---|---|")
        for p in ("bf16", "mxfp8"):
            say(f"| {p} | {dev[p][0]:.2e} | {dev[p][1]:.2e} |")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
