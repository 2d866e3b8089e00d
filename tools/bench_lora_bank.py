"""A bank of LoRA adaptations behind one base (HuggingFaceEncoderAdapt.lora_bank, Wav2Vec2Plan._bank_term, csrc/lora_bank.hip) on one MI355X, one
process, precision="bf16", random weights of the named geometries (nothing here speaks about a trained checkpoint's transcripts):
  * the graphed forward step at the C5 geometry (wav2vec2-large, 16 x 20 s) and the XLS-R 1B geometry (hidden 1280, 48 layers, head_dim 80, pre-LN)
    with a bank (r = 16 on q and v, 8 slots, clip i selects slot i mod 8) next to the same plan without one, in the order base, bank, base again --
    the two base timings show the run's spread;
  * the q | v launch (bf16 y, two slices of the [rows][3 c] buffer) and the out_proj-form launch (f32 y, ldy = c) per call, next to ts_lora_fwd at
    the same rows / k / n / r (f32 y, one target) in the same run, each next to its HBM floor: x once + y read and written + the banks.
python tools/bench_lora_bank.py [--batch 16] [--seconds 20] [--steps 30] [--rank 16] [--slots 8] [--layers-c5 24] [--layers-xlsr 48] [--out FILE.md]"""
import argparse
import os
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tools.bench_c5 import config, random_state
from tools.bench_mxfp8 import HBM_PEAK, _blocks
from tools.bench_wavlm import layer_norm_variant

TARGETS = ("q_proj", "v_proj")


def geometries(a):
    c5 = config(False, a.layers_c5)
    x1 = config(False, a.layers_xlsr)
    x1 = SimpleNamespace(**{**vars(x1), "hidden_size": 1280, "intermediate_size": 5120, "num_attention_heads": 16})
    x1, x1_sd = layer_norm_variant(x1, random_state(x1), False)
    return {"C5 (wav2vec2-large)": (c5, random_state(c5)), "XLS-R 1B": (x1, x1_sd)}


def random_bank(cfg, a):
    """A full bank with the statistics of a trained adaptation (A as lora_finetuning() draws it, B from N(0, 0.02)), clip i on slot i mod slots."""
    from thunder_speech_amd.huggingface.encoder import LoraBank
    c = int(cfg.hidden_size)
    bank = LoraBank(int(cfg.num_hidden_layers), c, a.rank, 2.0 * a.rank, TARGETS, a.slots, "bf16", "cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    bank.a_qkv.copy_((torch.rand(bank.a_qkv.shape, generator=g, device="cuda") * 2 - 1) / c ** 0.5)
    bank.b_qkv.copy_(0.02 * torch.randn(bank.b_qkv.shape, generator=g, device="cuda"))
    bank.scales.fill_(2.0)
    bank.names = [f"slot{i}" for i in range(a.slots)]
    bank.selection = [bank.names[i % a.slots] for i in range(a.batch)]
    bank.write_ids()
    return bank


def time_steps(cfg, sd, a):
    """-> ({label: ms / step}, frames, launches of one forward without and with the bank): one plan, one graph per launch sequence."""
    from thunder_speech_amd import _lib
    from thunder_speech_amd.huggingface.encoder import Wav2Vec2Plan
    from thunder_speech_amd.huggingface.transform import Wav2Vec2Preprocess
    pre = Wav2Vec2Preprocess()
    x = (0.1 * torch.randn(a.batch, 16000 * a.seconds, generator=torch.Generator().manual_seed(0))).cuda()
    lengths = torch.full((a.batch,), 16000 * a.seconds, dtype=torch.int32, device="cuda")
    res, runs, calls = {}, {}, {}
    with torch.no_grad():
        plan = Wav2Vec2Plan(cfg, sd, "cuda", precision="bf16")
        bank = random_bank(cfg, a)

        def step():
            xn, _ = pre(x, lengths)
            return plan.forward(xn, None)
        for label, b in (("base", None), ("bank", bank)):
            plan.bank = b
            out = step(); torch.cuda.synchronize()
            n0 = _lib.CALLS
            out = step(); torch.cuda.synchronize()
            calls[label] = _lib.CALLS - n0
            assert torch.isfinite(out).all(), label
            graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
            with torch.cuda.stream(side):
                with torch.cuda.graph(graph, stream=side):
                    gout = step()
            graph.replay(); torch.cuda.synchronize()
            if not torch.equal(gout, out):
                print(f"{label}: graph replay differs from the eager forward by {float((gout - out).abs().max()):.3g}")
            runs[label] = (graph, gout, out)
        moved = float((runs["bank"][2] - runs["base"][2]).abs().max())
        for label, key in (("base (first)", "base"), ("bank", "bank"), ("base (second)", "base")):
            run = runs[key][0].replay
            run(); run(); torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                run()
            torch.cuda.synchronize()
            res[label] = (time.perf_counter() - t0) / a.steps * 1e3
    frames = out.shape[1]
    del runs, plan, bank
    torch.cuda.empty_cache()
    return res, frames, calls, moved


def time_launches(rows_b, t, c, a, reps=100):
    """-> ({name: [us per block]}, {name: floor bytes}) at batch rows_b x t rows, k = n = c."""
    from thunder_speech_amd import _lib
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    bf, r, slots, rows = torch.bfloat16, a.rank, a.slots, rows_b * t
    g = torch.Generator().manual_seed(4)
    x16 = torch.randn(rows, c, generator=g).to(bf).cuda()
    qkv16 = torch.randn(rows, 3 * c, generator=g).to(bf).cuda()
    h, y3 = torch.randn(rows, c, generator=g).cuda(), torch.randn(rows, 3 * c, generator=g).cuda()
    a2 = (torch.randn(slots, 2, r, c, generator=g) / c ** 0.5).to(bf).cuda()
    b2 = torch.zeros(slots, 2, c, r, dtype=bf).cuda()              # a zero term: the repeated in-place launches leave y as it is
    a1, b1 = a2[:, :1].contiguous(), b2[:, :1].contiguous()
    scales = torch.full((slots,), 2.0, device="cuda")
    ids = (torch.arange(rows_b, dtype=torch.int32) % slots).cuda()
    u16 = torch.empty(rows, r, dtype=bf, device="cuda")
    calls = {
        "ts_lora_bank_fwd, q and v into bf16 [rows][3 c]": lambda: L.ts_lora_bank_fwd(
            x16.data_ptr(), 1, c, rows_b, t, c, a2.data_ptr(), b2.data_ptr(), scales.data_ptr(), slots, 2, c, r, ids.data_ptr(), qkv16.data_ptr(), 1,
            3 * c, 0, 2 * c, -1, s),
        "ts_lora_bank_fwd, out_proj form into f32 [rows][c]": lambda: L.ts_lora_bank_fwd(
            x16.data_ptr(), 1, c, rows_b, t, c, a1.data_ptr(), b1.data_ptr(), scales.data_ptr(), slots, 1, c, r, ids.data_ptr(), h.data_ptr(), 0, c,
            0, -1, -1, s),
        "ts_lora_fwd, one target into f32 [rows][3 c]": lambda: L.ts_lora_fwd(
            x16.data_ptr(), rows, c, a1.data_ptr(), b1.data_ptr(), c, r, 2.0, y3.data_ptr() + 4 * c, 3 * c, u16.data_ptr(), s),
    }
    pair = 2 * r * c * 2                                             # A and B of one slot and target, bf16
    floors = {"ts_lora_bank_fwd, q and v into bf16 [rows][3 c]": rows * c * (2 + 2 * 4) + slots * 2 * pair,
              "ts_lora_bank_fwd, out_proj form into f32 [rows][c]": rows * c * (2 + 8) + slots * pair,
              "ts_lora_fwd, one target into f32 [rows][3 c]": rows * c * (2 + 8) + pair}
    times = _blocks(calls, reps)
    del x16, qkv16, h, y3, a2, b2, a1, b1, u16
    torch.cuda.empty_cache()
    return times, floors


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seconds", type=int, default=20)
    ap.add_argument("--steps", type=int, default=30, help="timed graph replays per timing")
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--layers-c5", type=int, default=24)
    ap.add_argument("--layers-xlsr", type=int, default=48)
    ap.add_argument("--out", default=None, help="also write the tables (markdown) to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lora_bank: needs an MI355X")
    box = torch.cuda.get_device_name(0)
    lines = [f"one process on one {box}; precision=\"bf16\", {a.batch} x {a.seconds} s, random weights; bank: rank {a.rank} on {', '.join(TARGETS)}, "
             f"{a.slots} slots, scale 2, clip i selects slot i mod {a.slots}; graphed forward (front end + encoder), 2 warm-up replays, then {a.steps} "
             "timed replays by the host clock, in the order base, bank, base again", "",
             "| geometry | frames | base (first) ms | bank ms | base (second) ms | bank - mean base ms | base spread ms | launches base / bank | max abs change of the output |",
             "|---|---:|---:|---:|---:|---:|---:|---|---:|"]
    launch_lines = []
    for name, (cfg, sd) in geometries(a).items():
        res, frames, calls, moved = time_steps(cfg, sd, a)
        base = 0.5 * (res["base (first)"] + res["base (second)"])
        over = res["bank"] - base
        lines.append(f"| {name} | {frames} | {res['base (first)']:.2f} | {res['bank']:.2f} | {res['base (second)']:.2f} | {over:.2f} | "
                     f"{abs(res['base (first)'] - res['base (second)']):.2f} | {calls['base']} / {calls['bank']} | {moved:.3g} |")
        c, layers = int(cfg.hidden_size), int(cfg.num_hidden_layers)
        times, floors = time_launches(a.batch, frames, c, a)
        launch_lines += ["", f"{name}: rows = {a.batch} x {frames} = {a.batch * frames}, k = n = {c}, r = {a.rank}, {a.slots} slots (device events, 3 blocks "
                         f"of 100 launches, the three calls alternated); HBM floor at {HBM_PEAK / 1e12:.0f} TB/s: x once + y read and written + the banks:", "",
                         "| entry point | us per call (blocks) | best us | floor MB | HBM floor us | best / floor |", "|---|---|---:|---:|---:|---:|"]
        for k, us in times.items():
            launch_lines.append(f"| {k} | {' / '.join(f'{v:.1f}' for v in us)} | {min(us):.1f} | {floors[k] / 1e6:.1f} | {floors[k] / HBM_PEAK * 1e6:.1f} | "
                                f"{min(us) / (floors[k] / HBM_PEAK * 1e6):.2f} |")
        qv = min(times["ts_lora_bank_fwd, q and v into bf16 [rows][3 c]"])
        launch_lines += ["", f"{name}: {layers} layers x the q | v launch = {layers * qv / 1e3:.2f} ms per step by the per-call time; the step's overhead above is "
                         f"{over:.2f} ms"]
    text = "\n".join(lines + launch_lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
