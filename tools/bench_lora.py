"""LoRA fine-tuning of the attention projections (HuggingFaceEncoderAdapt.lora_finetuning, huggingface/train.py LoRALinear, csrc/lora_train.hip) next
to full fine-tuning, same run, same GPU, train_precision="bf16": ms per step and peak allocated memory at the XLS-R 1B geometry (48 layers, 1280
hidden, head_dim 80, no adapters) and at the wav2vec2-large geometry (24 layers, 1024 hidden, head_dim 64), 8 x 10 s, and the LoRA node's forward
and backward launches at the 1B row geometry next to their computed HBM floors.  Modelled on tools/bench_mms.py --train-adapters (its step, its
timing: 2 warm-up steps, then timed steps in 2 blocks between device events, inputs rotated over 3 batches).

python tools/bench_lora.py [--batch 8] [--seconds 10] [--steps 10] [--rank 16] [--out FILE.md]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tools.bench_mms import HBM_PEAK, _best_of_blocks, graph_nodes

GEOMETRIES = {"XLS-R 1B (48 layers, 1280 hidden, 16 heads, 5120 FFN)": dict(hidden_size=1280, num_hidden_layers=48, num_attention_heads=16, intermediate_size=5120),
              "wav2vec2-large (24 layers, 1024 hidden, 16 heads, 4096 FFN)": dict(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16,
                                                                                  intermediate_size=4096)}
TARGETS = ("q_proj", "v_proj")


def train_model(geom, seed=0):
    """transformers' Wav2Vec2Model (pre-LN, layer-norm convs), random weights, the dropouts / time masking of tools/bench_mms.py's fine-tuning recipe."""
    import transformers
    torch.manual_seed(seed)
    return transformers.Wav2Vec2Model(transformers.Wav2Vec2Config(
        feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True, hidden_dropout=0.1, attention_dropout=0.1, activation_dropout=0.1,
        feat_proj_dropout=0.1, layerdrop=0.0, mask_time_prob=0.05, mask_feature_prob=0.0, vocab_size=32, **geom))


def time_train_step(a, geom, lora: bool, rounds=2, n_inputs=3):
    """ms / step (per block), peak allocated bytes, node names, t and the number of trained parameters of one regime (tools/bench_mms.py::time_train_step)."""
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    adapt = HuggingFaceEncoderAdapt(train_model(geom), mask_input=True, train_precision="bf16").cuda().train()
    if lora:
        named = adapt.lora_finetuning(rank=a.rank, alpha=2.0 * a.rank, targets=TARGETS)
        with torch.no_grad():                                      # B away from zero: a step in the middle of training, not the first
            for n, p in named.items():
                if n.endswith("lora_B"):
                    p.normal_(0.0, 0.02)
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
        print(f"  block ({'LoRA' if lora else 'full'}): " + " ".join(f"{x:.1f}" for x in steps_ms) + " ms", flush=True)
        blocks.append(sum(steps_ms) / per)
        peak = max(peak, torch.cuda.max_memory_allocated())
    out = dict(blocks=blocks, peak=peak, nodes=state["nodes"], t=state["t"], trained=sum(p.numel() for p in params), steps=per * rounds)
    del adapt, opt, xs, params
    torch.cuda.empty_cache()
    return out


def lora_calls(rows, c=1280, r=16):
    """-> ({name: call}, {name: HBM floor bytes}, buffers to keep alive): one target, the middle slice of a [rows][3 c] buffer, dx asked for."""
    from thunder_speech_amd import _lib
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(4)
    bf = torch.bfloat16
    x16, dy16 = torch.randn(rows, c, generator=g).to(bf).cuda(), torch.randn(rows, 3 * c, generator=g).to(bf).cuda()
    a16 = (torch.randn(r, c, generator=g) / c ** 0.5).to(bf).cuda()
    b16 = torch.zeros(c, r, dtype=bf).cuda()                     # a zero term: the repeated in-place launches leave y and dx as they are
    at16, bt16 = a16.t().contiguous(), b16.t().contiguous()
    y, dx = torch.randn(rows, 3 * c, generator=g).cuda(), torch.randn(rows, c, generator=g).cuda()
    u16 = torch.empty(rows, r, dtype=bf, device="cuda")
    da, db = torch.empty(r, c, device="cuda"), torch.empty(c, r, device="cuda")
    ws = torch.empty(L.ts_lora_bwd_workspace(rows, c, c, r), dtype=torch.uint8, device="cuda")
    calls = {
        "ts_lora_fwd": lambda: L.ts_lora_fwd(x16.data_ptr(), rows, c, a16.data_ptr(), b16.data_ptr(), c, r, 2.0, y.data_ptr() + 4 * c, 3 * c, u16.data_ptr(), s),
        "ts_lora_bwd": lambda: L.ts_lora_bwd(dy16.data_ptr() + 2 * c, 3 * c, x16.data_ptr(), u16.data_ptr(), rows, c, c, r, 2.0, at16.data_ptr(),
                                             bt16.data_ptr(), dx.data_ptr(), da.data_ptr(), db.data_ptr(), ws.data_ptr(), s),
        "ts_lora_bwd, dx = NULL": lambda: L.ts_lora_bwd(dy16.data_ptr() + 2 * c, 3 * c, x16.data_ptr(), u16.data_ptr(), rows, c, c, r, 2.0, at16.data_ptr(),
                                                        bt16.data_ptr(), None, da.data_ptr(), db.data_ptr(), ws.data_ptr(), s),
    }
    floors = {"ts_lora_fwd": rows * c * (2 + 8), "ts_lora_bwd": rows * c * (2 + 2 + 8), "ts_lora_bwd, dx = NULL": rows * c * (2 + 2)}
    return calls, floors, (x16, dy16, a16, b16, at16, bt16, y, dx, u16, da, db, ws)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seconds", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10, help="timed steps per regime")
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--out", default=None, help="also write the tables (markdown) to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lora: needs an MI355X")
    lines = [f"fine-tuning step, train_precision=\"bf16\": {a.batch} x {a.seconds} s (one clip 3/4 long), pre-LN, layer-norm convs, random weights, dropouts 0.1 "
             f"(attention included), mask_time_prob 0.05; forward + backward of a probe loss + AdamW over the trained parameters; one process, 2 warm-up steps, "
             f"then {a.steps} timed steps in 2 blocks between device events, inputs rotated over 3 batches.  LoRA: rank {a.rank}, alpha {2 * a.rank}, targets "
             f"{', '.join(TARGETS)}, B drawn from N(0, 0.02)", "",
             "| geometry | regime | trained parameters | ms/step | blocks | peak allocated GiB |", "|---|---|---:|---:|---|---:|"]
    t_1b, verdicts, nodes = None, [], None
    for name, geom in GEOMETRIES.items():
        full = time_train_step(a, geom, lora=False)
        lo = time_train_step(a, geom, lora=True)
        ms = {}
        for regime, r in (("full fine-tuning", full), (f"LoRA r = {a.rank} on q, v", lo)):
            ms[regime] = sum(r["blocks"]) / len(r["blocks"])
            lines.append(f"| {name} | {regime} | {r['trained']:,} | {ms[regime]:.1f} | {' / '.join(f'{x:.1f}' for x in r['blocks'])} | {r['peak'] / 2 ** 30:.2f} |")
        m_full, m_lora = ms["full fine-tuning"], ms[f"LoRA r = {a.rank} on q, v"]
        verdicts.append(f"{name}: the LoRA step takes {m_lora / m_full:.3f} of the full step ({m_lora:.1f} ms against {m_full:.1f} ms: "
                        f"{'below it, as expected' if m_lora < m_full else 'NOT below it'}), peak memory {lo['peak'] / full['peak']:.3f} of it")
        if t_1b is None:
            t_1b, nodes = lo["t"], lo["nodes"]
    lines += [""] + verdicts
    lines += ["", "autograd nodes of one LoRA step's graph at the 1B geometry (name x count): " + ", ".join(f"{nm} x {cnt}" for nm, cnt in sorted(nodes.items()))]
    rows = a.batch * t_1b
    calls, floors, keep = lora_calls(rows, r=a.rank)
    best = _best_of_blocks(calls, 20)
    lines += ["", f"LoRA node launches, one target, rows = {a.batch} x {t_1b} = {rows}, k = n = 1280, r = {a.rank}, the target the middle slice of a [rows][3 c] buffer "
              f"(device events, best of 3 blocks of 20); HBM floor at {HBM_PEAK / 1e12:.0f} TB/s: forward x16 + the read-modify-write of the f32 slice (rows c 10 "
              "bytes), backward dy16 + x16 + the read-modify-write of dx (rows c 12 bytes), without dx dy16 + x16 (rows c 4 bytes):", "",
              "| entry point | us per call | floor MB | HBM floor us | achieved TB/s of the floor's bytes |", "|---|---:|---:|---:|---:|"]
    for k, us in best.items():
        lines.append(f"| {k} | {us:.1f} | {floors[k] / 1e6:.1f} | {floors[k] / HBM_PEAK * 1e6:.1f} | {floors[k] / us / 1e6:.2f} |")
    lines += ["", f"one target per call: q and v of a node read x16 once each, {rows * 1280 * 2 / 1e6:.1f} MB a target more than a joint launch would "
              f"({rows * 1280 * 2 / HBM_PEAK * 1e6:.1f} us at the HBM peak); per step and layer the node adds 2 forward and 2 backward calls"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
