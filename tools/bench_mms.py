"""MMS-1B inference on the HIP path (random weights): hidden 1280, 48 layers, 16 heads (head_dim 80), FFN 5120, layer-norm convs, pre-LN,
adapter_attn_dim 16; 16 x 20 s, bf16 -- eager and graphed, next to the same geometry without adapters (XLS-R 1B) -- and the per-launch times of
the two launches of csrc/mms.hip at that step's geometry (t = 999 frames):
  ts_mms_attention_fwd     against ts_w2v_attention_fwd on the same head_dim-80 input (which materialises the [t][t] scores)
  ts_mms_attn_adapter_fwd  (adapter + the LayerNorm behind it) against a plain ts_w2v_layernorm_fwd over the same rows, next to its HBM floor
python tools/bench_mms.py [--batch 16] [--seconds 20] [--layers 48] [--steps 5] [--out FILE.md]

--train: mixed-precision fine-tuning steps (train_precision="bf16": training forward, backward of a probe loss, AdamW) at the XLS-R 1B geometry
without adapters, 8 x 10 s, attention dropout 0.1, with the fused head_dim 80 attention node (huggingface/train.py AttentionFused80,
csrc/mms_train.hip, csrc/w2v_attn_train.hip) and with train.FUSED_ATTENTION = False (the materialised `Attention` node) -- same process, alternating blocks, device events,
rotated inputs, peak allocated memory of both -- and the per-call times of ts_mms_attention_train_fwd / _bwd at that step's t next to the
head_dim 64 calls at the same batch, t and heads (c = 1024).
python tools/bench_mms.py --train [--batch 8] [--seconds 10] [--layers 48] [--steps 10] [--out FILE.md]
--train-kernels: only issues those launches, for a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/bench_mms.py --train-kernels):
the four launches of the head_dim 80 path are attn_fwd_train_kernel<80>, attn_rowdot80_kernel, attn_bwd_dq_kernel<80> and attn_bwd_dkv_kernel<80>.

--train-adapters: adapter-only fine-tuning of the MMS-1B geometry (adapter_attn_dim 16, HuggingFaceEncoderAdapt.adapter_finetuning(): the base frozen,
the 48 attention adapters trained; huggingface/train.py AttnAdapter, csrc/mms_adapter_train.hip), 8 x 10 s, train_precision="bf16" -- ms per step
and peak allocated memory next to the full fine-tuning step of the same geometry without adapters, same process -- and the per-call times of
ts_mms_attn_adapter_train_fwd / _bwd at that step's rows next to their HBM floor and to transformers' own Wav2Vec2AttnAdapterLayer + residual,
forward + backward under torch on the same GPU.  The fused pair taking longer than torch's is an error (exit status 1).
python tools/bench_mms.py --train-adapters [--batch 8] [--seconds 10] [--layers 48] [--steps 10] [--out FILE.md]"""
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
        "ts_mms_attention_fwd (w2v_flash_attn_kernel<80>)": lambda: L.ts_mms_attention_fwd(qkv.data_ptr(), b, t, c, heads, None, ctx.data_ptr(), s),
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


def train_model(layers, seed=0, adapter_attn_dim=None):
    """transformers' Wav2Vec2Model at the XLS-R 1B geometry (pre-LN, layer-norm convs; adapter_attn_dim: MMS-1B's attention adapters), random weights,
    attention dropout 0.1 and the other dropouts / time masking of tools/bench_wavlm.py's fine-tuning recipe."""
    import transformers
    torch.manual_seed(seed)
    return transformers.Wav2Vec2Model(transformers.Wav2Vec2Config(
        hidden_size=1280, num_hidden_layers=layers, num_attention_heads=16, intermediate_size=5120, feat_extract_norm="layer",
        do_stable_layer_norm=True, conv_bias=True, hidden_dropout=0.1, attention_dropout=0.1, activation_dropout=0.1, feat_proj_dropout=0.1,
        layerdrop=0.0, mask_time_prob=0.05, mask_feature_prob=0.0, vocab_size=32, adapter_attn_dim=adapter_attn_dim))


def graph_nodes(fn):
    """{autograd node name: count} of the graph behind grad_fn `fn`."""
    seen, todo, names = set(), [fn], {}
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        names[type(f).__name__] = names.get(type(f).__name__, 0) + 1
        todo += [g for g, _ in f.next_functions]
    return names


def time_train_ab(a, rounds=2, n_inputs=3):
    """ms / step and peak allocated bytes of the fine-tuning step with train.FUSED_ATTENTION on and off: one model, one optimizer, one process;
    2 warm-up steps per mode, then `rounds` alternating blocks of steps / rounds timed steps per mode between device events; the inputs rotate
    over `n_inputs` seeded batches.  -> ({mode: [ms / step of each block]}, {mode: bytes}, {mode: node names}, t, timed steps per mode)"""
    from thunder_speech_amd.huggingface import train as T
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    adapt = HuggingFaceEncoderAdapt(train_model(a.layers), mask_input=True, train_precision="bf16").cuda().train()
    opt = torch.optim.AdamW([p for p in adapt.parameters() if p.requires_grad], lr=1e-5)
    g = torch.Generator().manual_seed(0)
    xs = [(0.1 * torch.randn(a.batch, 16000 * a.seconds, generator=g)).cuda() for _ in range(n_inputs)]
    lengths = torch.full((a.batch,), 16000 * a.seconds, dtype=torch.int64, device="cuda")
    lengths[-1] = 16000 * a.seconds * 3 // 4                                  # one ragged clip
    state = dict(probe=None, i=0, nodes=None, t=None)

    def step(walk=False):
        opt.zero_grad(set_to_none=True)
        feats, _ = adapt(xs[state["i"] % n_inputs], lengths)
        state["i"] += 1
        if state["probe"] is None:
            state["probe"], state["t"] = torch.randn(feats.shape, generator=g).cuda(), feats.shape[-1]
        if walk:
            state["nodes"] = graph_nodes(feats.grad_fn)
        (feats * state["probe"]).mean().backward()
        opt.step()

    modes = {"fused (AttentionFused80)": True, "FUSED_ATTENTION = False (Attention)": False}
    per = max(1, (a.steps + rounds - 1) // rounds)
    blocks, peak, nodes = {k: [] for k in modes}, {k: 0 for k in modes}, {}
    old = T.FUSED_ATTENTION
    try:
        for k, on in modes.items():
            T.FUSED_ATTENTION = on
            for i in range(2):
                step(walk=i == 0)
            nodes[k] = state["nodes"]
        torch.cuda.synchronize()
        for _ in range(rounds):
            for k, on in modes.items():
                T.FUSED_ATTENTION = on
                # the caching allocator keeps its blocks: emptying it here would put the re-allocations of the block's first step into the timed window
                torch.cuda.reset_peak_memory_stats()
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(per + 1)]
                ev[0].record()
                for i in range(per):
                    step()
                    ev[i + 1].record()
                torch.cuda.synchronize()
                steps_ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(per)]
                print(f"  block of {k}: " + " ".join(f"{x:.1f}" for x in steps_ms) + " ms", flush=True)
                blocks[k].append(sum(steps_ms) / per)
                peak[k] = max(peak[k], torch.cuda.max_memory_allocated())
    finally:
        T.FUSED_ATTENTION = old
    t = state["t"]
    del adapt, opt, xs
    torch.cuda.empty_cache()
    return blocks, peak, nodes, t, per * rounds


def train_attention_calls(a, t, heads=16, p=0.1):
    """{name: call} of the fused training attention at head_dim 80 and 64, same batch, t and heads; the backward is given the forward's mask, so a
    forward call is the mask draw + the forward kernel and a backward call is the row-dot, dQ and dKV launches."""
    from thunder_speech_amd import _lib
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(3)
    calls = {}
    keep = []
    for hd, entry in ((80, "ts_mms_attention_train"), (64, "ts_w2v_attention_train")):
        b, c = a.batch, hd * heads
        q16 = torch.randn(b, t, 3 * c, generator=g).to(torch.bfloat16).cuda()
        dout = torch.randn(b, t, c, generator=g).cuda()
        ctx, lse2, dq = torch.empty(b, t, c, device="cuda"), torch.empty(b, heads, t, device="cuda"), torch.empty(b, t, 3 * c, device="cuda")
        wf = torch.empty(getattr(L, entry + "_fwd_workspace")(b, t, c, heads), dtype=torch.uint8, device="cuda")
        wb = torch.empty(getattr(L, entry + "_bwd_workspace")(b, t, c, heads), dtype=torch.uint8, device="cuda")
        keep.append((q16, dout, ctx, lse2, dq, wf, wb))
        fwd, bwd = getattr(L, entry + "_fwd"), getattr(L, entry + "_bwd")
        calls[f"{entry}_fwd (head_dim {hd})"] = (lambda fwd=fwd, q16=q16, b=b, c=c, ctx=ctx, lse2=lse2, wf=wf:
                                                 fwd(q16.data_ptr(), b, t, c, heads, None, p, 7, ctx.data_ptr(), lse2.data_ptr(), wf.data_ptr(), s))
        calls[f"{entry}_bwd (head_dim {hd})"] = (lambda bwd=bwd, q16=q16, b=b, c=c, ctx=ctx, lse2=lse2, wf=wf, dout=dout, dq=dq, wb=wb:
                                                 bwd(q16.data_ptr(), b, t, c, heads, None, p, 7, dout.data_ptr(), ctx.data_ptr(), lse2.data_ptr(),
                                                     wf.data_ptr(), dq.data_ptr(), wb.data_ptr(), s))
    return calls, keep


def main_train(a):
    blocks, peak, nodes, t, n = time_train_ab(a)
    ms = {k: sum(v) / len(v) for k, v in blocks.items()}
    plain = list(ms)[1]
    lines = [f"fine-tuning step, train_precision=\"bf16\": {a.batch} x {a.seconds} s (one clip 3/4 long), {a.layers} layers, 1280 hidden / 16 heads (head_dim 80) / "
             f"5120 FFN, pre-LN, layer-norm convs, no adapters, random weights, t = {t} frames, dropouts 0.1 (attention included), mask_time_prob 0.05; "
             f"forward + backward + AdamW; one process, 2 warm-up steps per mode, then {n} timed steps per mode in alternating blocks between device "
             "events, inputs rotated over 3 batches", "",
             "| attention node | ms/step | blocks | vs FUSED_ATTENTION = False | peak allocated GiB |", "|---|---:|---|---:|---:|"]
    for k in ms:
        lines.append(f"| {k} | {ms[k]:.1f} | {' / '.join(f'{x:.1f}' for x in blocks[k])} | {ms[k] / ms[plain]:.3f} | {peak[k] / 2 ** 30:.2f} |")
    lines += ["", "autograd nodes of one step's graph (name x count):", ""]
    for k in ms:
        lines.append(f"- {k}: " + ", ".join(f"{nm} x {cnt}" for nm, cnt in sorted(nodes[k].items())))
    calls, keep = train_attention_calls(a, t)
    best = _best_of_blocks(calls, 20)
    lines += ["", f"fused training attention calls, {a.batch} clips x 16 heads x t = {t}, p = 0.1, the backward given the forward's mask (device events, best of 3 "
              "blocks of 20); a forward call = mask draw + forward kernel, a backward call = row-dot + dQ + dKV launches:", "",
              "| entry point | us per call | vs head_dim 64 |", "|---|---:|---:|"]
    for k, us in best.items():
        ref = best[k.replace("ts_mms_attention_train", "ts_w2v_attention_train").replace("head_dim 80", "head_dim 64")]
        lines.append(f"| {k} | {us:.1f} | {us / ref:.3f} |")
    return lines


def time_train_step(a, adapters: bool, rounds=2, n_inputs=3):
    """ms / step (per block), peak allocated bytes, node names, t and the number of trained parameters of one fine-tuning regime: adapters = True --
    MMS-1B geometry, adapter_finetuning() (base frozen); False -- the same geometry without adapters, everything behind the conv front end trained.
    2 warm-up steps, then `rounds` blocks of steps / rounds timed steps between device events; the inputs rotate over `n_inputs` seeded batches."""
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    adapt = HuggingFaceEncoderAdapt(train_model(a.layers, adapter_attn_dim=16 if adapters else None), mask_input=True, train_precision="bf16").cuda().train()
    if adapters:
        adapt.adapter_finetuning(init=True)
    params = [p for p in adapt.parameters() if p.requires_grad]
    opt = torch.optim.AdamW(params, lr=1e-5)
    g = torch.Generator().manual_seed(0)
    xs = [(0.1 * torch.randn(a.batch, 16000 * a.seconds, generator=g)).cuda() for _ in range(n_inputs)]
    lengths = torch.full((a.batch,), 16000 * a.seconds, dtype=torch.int64, device="cuda")
    lengths[-1] = 16000 * a.seconds * 3 // 4                                  # one ragged clip
    state = dict(probe=None, i=0, nodes=None, t=None)

    def step(walk=False):
        opt.zero_grad(set_to_none=True)
        feats, _ = adapt(xs[state["i"] % n_inputs], lengths)
        state["i"] += 1
        if state["probe"] is None:
            state["probe"], state["t"] = torch.randn(feats.shape, generator=g).cuda(), feats.shape[-1]
        if walk:
            state["nodes"] = graph_nodes(feats.grad_fn)
        (feats * state["probe"]).mean().backward()
        opt.step()

    for i in range(2):
        step(walk=i == 0)
    torch.cuda.synchronize()
    per = max(1, (a.steps + rounds - 1) // rounds)
    blocks, peak = [], 0
    for _ in range(rounds):
        torch.cuda.reset_peak_memory_stats()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(per + 1)]
        ev[0].record()
        for i in range(per):
            step()
            ev[i + 1].record()
        torch.cuda.synchronize()
        steps_ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(per)]
        print(f"  block ({'adapter-only' if adapters else 'full'}): " + " ".join(f"{x:.1f}" for x in steps_ms) + " ms", flush=True)
        blocks.append(sum(steps_ms) / per)
        peak = max(peak, torch.cuda.max_memory_allocated())
    out = dict(blocks=blocks, peak=peak, nodes=state["nodes"], t=state["t"], trained=sum(p.numel() for p in params), steps=per * rounds)
    del adapt, opt, xs, params
    torch.cuda.empty_cache()
    return out


def adapter_train_calls(rows, c=1280, ad=16):
    """-> ({name: call}, torch's forward + backward as a callable, buffers to keep alive) at precision 1, dh asked for."""
    import transformers
    from transformers.models.wav2vec2.modeling_wav2vec2 import Wav2Vec2AttnAdapterLayer
    from thunder_speech_amd import _lib
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(4)
    h, dy = torch.randn(rows, c, generator=g).cuda(), torch.randn(rows, c, generator=g).cuda()
    layer = Wav2Vec2AttnAdapterLayer(transformers.Wav2Vec2Config(hidden_size=c, adapter_attn_dim=ad)).cuda()
    with torch.no_grad():
        layer.linear_2.weight.copy_(0.02 * torch.randn(c, ad, generator=g))
    nw, nb, b1, b2 = (t.detach() for t in (layer.norm.weight, layer.norm.bias, layer.linear_1.bias, layer.linear_2.bias))
    w1, w2 = layer.linear_1.weight.detach().to(torch.bfloat16), layer.linear_2.weight.detach().to(torch.bfloat16)
    y, dh = torch.empty_like(h), torch.empty_like(h)
    grads = [torch.empty_like(t, dtype=torch.float32) for t in (nw, nb, w1, b1, w2, b2)]
    ws = torch.empty(L.ts_mms_attn_adapter_train_bwd_workspace(rows, c, ad), dtype=torch.uint8, device="cuda")
    calls = {
        "ts_mms_attn_adapter_train_fwd": lambda: L.ts_mms_attn_adapter_train_fwd(h.data_ptr(), rows, c, ad, nw.data_ptr(), nb.data_ptr(), w1.data_ptr(),
                                                                                 b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), y.data_ptr(), 1, s),
        "ts_mms_attn_adapter_train_bwd": lambda: L.ts_mms_attn_adapter_train_bwd(h.data_ptr(), dy.data_ptr(), rows, c, ad, nw.data_ptr(), nb.data_ptr(),
                                                                                 w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), dh.data_ptr(),
                                                                                 *(t.data_ptr() for t in grads), ws.data_ptr(), 1, s),
    }
    hg = h.clone().requires_grad_(True)
    inputs = [hg] + list(layer.parameters())

    def torch_pair(autocast):
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            out = hg + layer(hg)
        torch.autograd.grad(out, inputs, dy)
    return calls, torch_pair, (h, dy, y, dh, grads, ws, layer, hg)


def time_adapter_train(a, t, reps=20):
    rows = a.batch * t
    calls, torch_pair, keep = adapter_train_calls(rows)
    best = _best_of_blocks(calls, reps)
    ref = {}
    for name, autocast in (("torch, f32", False), ("torch, autocast bf16", True)):
        ref[name] = float("inf")
        for _ in range(3):
            torch_pair(autocast)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                torch_pair(autocast)
            e1.record(); torch.cuda.synchronize()
            ref[name] = min(ref[name], e0.elapsed_time(e1) / reps * 1e3)
    return best, ref, rows


def main_train_adapters(a):
    """-> (markdown lines, whether the fused pair is no slower than torch's)"""
    full = time_train_step(a, adapters=False)
    ad = time_train_step(a, adapters=True)
    t = ad["t"]
    lines = [f"fine-tuning step, train_precision=\"bf16\": {a.batch} x {a.seconds} s (one clip 3/4 long), {a.layers} layers, 1280 hidden / 16 heads (head_dim 80) / "
             f"5120 FFN, pre-LN, layer-norm convs, random weights, t = {t} frames, dropouts 0.1 (attention included), mask_time_prob 0.05; forward + backward of "
             f"a probe loss + AdamW over the trained parameters; one process, 2 warm-up steps, then {ad['steps']} timed steps in 2 blocks between device "
             "events, inputs rotated over 3 batches", "",
             "| regime | trained parameters | ms/step | blocks | peak allocated GiB |", "|---|---:|---:|---|---:|"]
    for name, r in (("full fine-tuning, no adapters (XLS-R 1B geometry)", full), ("adapter-only, adapter_attn_dim 16 (MMS-1B geometry)", ad)):
        ms = sum(r["blocks"]) / len(r["blocks"])
        lines.append(f"| {name} | {r['trained']:,} | {ms:.1f} | {' / '.join(f'{x:.1f}' for x in r['blocks'])} | {r['peak'] / 2 ** 30:.2f} |")
    lines += ["", "autograd nodes of one adapter-only step's graph (name x count): " +
              ", ".join(f"{nm} x {cnt}" for nm, cnt in sorted(ad["nodes"].items()))]
    best, ref, rows = time_adapter_train(a, t)
    floor = {"ts_mms_attn_adapter_train_fwd": 2 * rows * 1280 * 4 / HBM_PEAK * 1e6, "ts_mms_attn_adapter_train_bwd": 3 * rows * 1280 * 4 / HBM_PEAK * 1e6}
    lines += ["", f"adapter node calls, rows = {a.batch} x {t} = {rows}, c = 1280, a = 16, precision 1, dh asked for (device events, best of 3 blocks of 20); HBM "
              f"floor at {HBM_PEAK / 1e12:.0f} TB/s: forward 2 rows c 4 bytes (read h, write y), backward 3 rows c 4 (read h, read dy, write dh):", "",
              "| entry point | us per call | HBM floor us |", "|---|---:|---:|"]
    for k, us in best.items():
        lines.append(f"| {k} | {us:.1f} | {floor[k]:.1f} |")
    pair = sum(best.values())
    lines += ["", "forward + backward of the adapter with its residual, same rows, same GPU, same run; torch = transformers' Wav2Vec2AttnAdapterLayer under "
              "autograd (LayerNorm, Linear, ReLU, Linear, add: u, z, r and the term stored and read back):", "",
              "| path | us per forward + backward | vs the fused pair |", "|---|---:|---:|",
              f"| fused pair (ts_mms_attn_adapter_train_fwd + _bwd) | {pair:.1f} | 1.000 |"]
    for k, us in ref.items():
        lines.append(f"| {k} | {us:.1f} | {us / pair:.3f} |")
    ok = pair <= min(ref.values())
    lines += ["", f"the fused pair takes {'no longer' if ok else 'LONGER'} than torch's faster path ({pair:.1f} us against {min(ref.values()):.1f} us)"]
    return lines, ok


def main_train_kernels(a, t=499, reps=10):
    from thunder_speech_amd import _lib
    calls, keep = train_attention_calls(a, t)
    for _ in range(reps):
        for k, f in calls.items():
            _lib.check(f(), k)
    torch.cuda.synchronize()
    print(f"issued {reps} x {list(calls)} at batch {a.batch}, t = {t}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=None, help="default 16 (inference), 8 (--train)")
    ap.add_argument("--seconds", type=int, default=None, help="default 20 (inference), 10 (--train)")
    ap.add_argument("--layers", type=int, default=48)
    ap.add_argument("--steps", type=int, default=None, help="timed steps per mode: default 5 (inference), 10 (--train)")
    ap.add_argument("--train", action="store_true", help="mixed-precision fine-tuning steps, fused attention on and off, instead of inference")
    ap.add_argument("--train-kernels", action="store_true", help="only issue the training attention launches at t = 499 (for a kernel trace)")
    ap.add_argument("--train-adapters", action="store_true", help="adapter-only fine-tuning steps of the MMS-1B geometry next to full fine-tuning, and the "
                    "adapter node's calls against torch")
    ap.add_argument("--out", default=None, help="also write the tables (markdown) to this file")
    a = ap.parse_args()
    training = a.train or a.train_kernels or a.train_adapters
    a.batch = a.batch or (8 if training else 16)
    a.seconds = a.seconds or (10 if training else 20)
    a.steps = a.steps or (10 if training else 5)
    if not torch.cuda.is_available():
        raise SystemExit("bench_mms: needs an MI355X")
    if a.train_kernels:
        return main_train_kernels(a)
    if a.train or a.train_adapters:
        lines, ok = main_train_adapters(a) if a.train_adapters else (main_train(a), True)
        text = "\n".join(lines)
        print(text)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text + "\n")
        if not ok:
            raise SystemExit(1)
        return
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
