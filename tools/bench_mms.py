"""MMS-1B inference on the HIP path (random weights): hidden 1280, 48 layers, 16 heads (head_dim 80), FFN 5120, layer-norm convs, pre-LN,
adapter_attn_dim 16; 16 x 20 s, bf16 -- eager and graphed, next to the same geometry without adapters (XLS-R 1B) -- and the per-launch times of
the two kernels of csrc/mms.hip at that step's geometry (t = 999 frames):
  ts_mms_attention_fwd     against ts_w2v_attention_fwd on the same head_dim-80 input (which materialises the [t][t] scores)
  ts_mms_attn_adapter_fwd  (adapter + the LayerNorm behind it) against a plain ts_w2v_layernorm_fwd over the same rows, next to its HBM floor
python tools/bench_mms.py [--batch 16] [--seconds 20] [--layers 48] [--steps 5] [--out FILE.md]"""
import argparse
import os
import sys
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tools.bench_c5 import config, random_state
from tools.bench_wavlm import layer_norm_variant, time_model

HBM_PEAK = 8.0e12          # bytes / s, MI355X data sheet


def mms_variant(layers: int, adapters: bool, seed=2):
    """cfg / state dict at the MMS-1B geometry on bench_c5's random weights; `adapters`: adapter_attn_dim 16 with an adapter term of the order of
    the residual stream (transformers' initialisation leaves it near zero)."""
    cfg = config(False, layers)
    cfg = SimpleNamespace(**{**vars(cfg), "hidden_size": 1280, "intermediate_size": 5120, "num_attention_heads": 16})
    cfg, sd = layer_norm_variant(cfg, random_state(cfg), False)
    cfg.adapter_attn_dim = 16 if adapters else None
    if adapters:
        g = torch.Generator().manual_seed(seed)
        for i in range(layers):
            p = f"encoder.layers.{i}.adapter_layer."
            sd[p + "norm.weight"], sd[p + "norm.bias"] = torch.ones(1280), torch.zeros(1280)
            sd[p + "linear_1.weight"], sd[p + "linear_1.bias"] = torch.randn(16, 1280, generator=g) / 1280 ** 0.5, torch.zeros(16)
            sd[p + "linear_2.weight"], sd[p + "linear_2.bias"] = 0.02 * torch.randn(1280, 16, generator=g), torch.zeros(1280)
    return cfg, sd


def _best_of_blocks(calls, reps):
    """Per-launch device time (us) of each call, alternated in three blocks: the best block per call."""
    from thunder_speech_amd import _lib
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


def time_attention(a, t=999, heads=16, reps=20):
    from thunder_speech_amd import _lib
    L = _lib.lib()
    b, c = a.batch, 80 * heads
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(b, t, 3 * c, generator=g).to(torch.bfloat16).cuda()
    ctx = torch.empty(b, t, c, dtype=torch.bfloat16, device="cuda")
    ws_bytes = L.ts_w2v_attention_workspace_bytes(b, t, heads, 1)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    calls = {
        "ts_w2v_attention_fwd, head_dim 80 (materialised scores)": lambda: L.ts_w2v_attention_fwd(qkv.data_ptr(), b, t, c, heads, None, 1, ctx.data_ptr(),
                                                                                                   ws.data_ptr(), s),
        "ts_mms_attention_fwd (mms_flash_attn_kernel)": lambda: L.ts_mms_attention_fwd(qkv.data_ptr(), b, t, c, heads, None, ctx.data_ptr(), s),
    }
    return _best_of_blocks(calls, reps), ws_bytes


def time_adapter(a, t=999, c=1280, ad=16, reps=50):
    from thunder_speech_amd import _lib
    L = _lib.lib()
    rows = a.batch * t
    g = torch.Generator().manual_seed(4)
    h = torch.randn(rows, c, generator=g).cuda()
    ones, zeros = torch.ones(c).cuda(), torch.zeros(c).cuda()
    w1, b1 = (torch.randn(ad, c, generator=g) / c ** 0.5).to(torch.bfloat16).cuda(), torch.zeros(ad).cuda()
    w2 = torch.zeros(c, ad, dtype=torch.bfloat16).cuda()           # a zero term: the repeated in-place launches leave h as it is
    y16 = torch.empty(rows, c, dtype=torch.bfloat16, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    calls = {
        "ts_w2v_layernorm_fwd (bf16 result)": lambda: L.ts_w2v_layernorm_fwd(h.data_ptr(), None, None, ones.data_ptr(), zeros.data_ptr(), 1e-5, rows, c, 0,
                                                                             None, y16.data_ptr(), s),
        "ts_mms_attn_adapter_fwd + LayerNorm (bf16 result)": lambda: L.ts_mms_attn_adapter_fwd(
            h.data_ptr(), rows, c, ad, ones.data_ptr(), zeros.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), zeros.data_ptr(), ones.data_ptr(),
            zeros.data_ptr(), 1e-5, None, y16.data_ptr(), 1, s),
    }
    floors = {"ts_w2v_layernorm_fwd (bf16 result)": rows * (4 * c + 2 * c) / HBM_PEAK * 1e6,
              "ts_mms_attn_adapter_fwd + LayerNorm (bf16 result)": rows * (4 * c + 4 * c + 2 * c) / HBM_PEAK * 1e6}
    return _best_of_blocks(calls, reps), floors, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seconds", type=int, default=20)
    ap.add_argument("--layers", type=int, default=48)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the tables (markdown) to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mms: needs an MI355X")
    rows, t = [], None
    for name, adapters in (("XLS-R 1B geometry (no adapters)", False), ("MMS-1B (adapter_attn_dim 16)", True)):
        r, t = time_model(name, *mms_variant(a.layers, adapters), a)
        rows.append((name, r))
    base = rows[0][1]
    lines = [f"{a.batch} x {a.seconds} s, {a.layers} layers, 1280 hidden / 16 heads (head_dim 80) / 5120 FFN, layer-norm convs, pre-LN, bf16, t = {t} frames; "
             f"{a.steps} timed steps per mode after warm-up", "",
             "| model | eager ms/step | graphed ms/step | graphed vs no adapters |", "|---|---:|---:|---:|"]
    for name, r in rows:
        lines.append(f"| {name} | {r['eager']:.1f} | {r['graphed']:.1f} | {r['graphed'] / base['graphed']:.3f} |")
    att, ws_bytes = time_attention(a)
    ref = att["ts_w2v_attention_fwd, head_dim 80 (materialised scores)"]
    lines += ["", f"attention core, {a.batch} clips x 16 heads x t = 999, head_dim 80, bf16 (device events, best of 3 blocks of 20); the materialised path's "
              f"workspace at this geometry is {ws_bytes / 2 ** 20:.0f} MiB, the fused kernel has none:", "",
              "| entry point | us per launch | vs materialised |", "|---|---:|---:|"]
    for k, us in att.items():
        lines.append(f"| {k} | {us:.1f} | {us / ref:.3f} |")
    ad, floors, nrows = time_adapter(a)
    ln = ad["ts_w2v_layernorm_fwd (bf16 result)"]
    lines += ["", f"adapter launch, {nrows} rows x 1280, a = 16, precision 1 (device events, best of 3 blocks of 50); HBM floor = the launch's own row traffic "
              f"at {HBM_PEAK / 1e12:.0f} TB/s (LayerNorm: read 4c, write 2c bytes per row; adapter + LayerNorm: read 4c, write 4c + 2c):", "",
              "| entry point | us per launch | HBM floor us | vs plain LayerNorm |", "|---|---:|---:|---:|"]
    for k, us in ad.items():
        lines.append(f"| {k} | {us:.1f} | {floors[k]:.1f} | {us / ln:.3f} |")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
