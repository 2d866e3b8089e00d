"""Many MMS languages on one base (BaseCTCModule.language_bank, huggingface/language_bank.py, csrc/mms_lang_bank.hip) on one MI355X, one process,
precision="bf16", random weights at the MMS-1B geometry (hidden 1280, 48 layers, 16 heads, FFN 5120, adapter_attn_dim 16), synthetic audio:
  * the graphed step -- waveform normalisation, encoder, CTC head -- without a bank (the layers' own adapters, the linear decoder), with a bank and
    every clip on slot 0, and with a bank of 8 languages and clip i on slot i mod 8: ONE graph serves both selections; timed in the order
    no bank, slot 0, mixed, no bank again -- the two bank-less timings show the run's spread;
  * ts_mms_lang_bank_adapter_fwd next to ts_mms_attn_adapter_fwd on the same rows, and ts_mms_lang_bank_head_fwd next to the linear decoder's eval
    forward (bf16 packing + the TCS pointwise head) it replaces, each next to its HBM floor, computed from the shapes below.
The tool needs the GPU and does not fall back.
python tools/bench_mms_lang_bank.py [--batch 16] [--seconds 20] [--layers 48] [--steps 20] [--slots 8] [--vocab 154] [--out FILE.md]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tools.bench_mms import HBM_PEAK, mms_variant
from tools.bench_mxfp8 import _blocks

C, A = 1280, 16


def random_bank(plan, sd, decoder, a):
    """A full bank: slot 0 the plan's own adapters and `decoder`, the other slots random languages with vocabularies of different sizes."""
    from thunder_speech_amd.huggingface.language_bank import LanguageBank
    v_pad = -(-a.vocab // 16) * 16
    bank = LanguageBank(a.layers, C, A, a.slots, v_pad, "bf16", "cuda")
    lin = decoder[2]
    bank.write_slot(0, "lang0", [sd[k] for k in plan.attn_adapter_keys], lin.weight, lin.bias, None)
    g = torch.Generator().manual_seed(5)
    for s in range(1, a.slots):
        ad = []
        for _ in range(a.layers):
            ad += [1.0 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g), torch.randn(A, C, generator=g) / C ** 0.5,
                   0.1 * torch.randn(A, generator=g), 0.02 * torch.randn(C, A, generator=g), 0.1 * torch.randn(C, generator=g)]
        n = max(16, a.vocab - 9 * s)
        bank.write_slot(s, f"lang{s}", ad, torch.randn(n, C, generator=g) / C ** 0.5, torch.zeros(n), None)
    return bank


def time_steps(a):
    """-> ({label: ms / step}, frames, {label: C-ABI calls of one step}, notes)"""
    from thunder_speech_amd import _lib
    from thunder_speech_amd.blocks import linear_decoder
    from thunder_speech_amd.huggingface.encoder import Wav2Vec2Plan
    from thunder_speech_amd.huggingface.transform import Wav2Vec2Preprocess
    cfg, sd = mms_variant(a.layers, True)
    pre = Wav2Vec2Preprocess()
    x = (0.1 * torch.randn(a.batch, 16000 * a.seconds, generator=torch.Generator().manual_seed(0))).cuda()
    lengths = torch.full((a.batch,), 16000 * a.seconds, dtype=torch.int32, device="cuda")
    res, runs, calls, notes = {}, {}, {}, []
    with torch.no_grad():
        plan = Wav2Vec2Plan(cfg, sd, "cuda", precision="bf16")
        torch.manual_seed(3)
        decoder = linear_decoder(C, a.vocab, decoder_dropout=0.0).cuda().eval()
        bank = random_bank(plan, sd, decoder, a)

        def step(b):
            plan.lang_bank = b
            xn, _ = pre(x, lengths)
            h = plan.forward(xn, None)
            return h, (decoder(h.transpose(-1, -2)) if b is None else b.head(h))
        for label, b in (("no bank", None), ("bank", bank)):
            out = step(b); torch.cuda.synchronize()
            n0 = _lib.CALLS
            out = step(b); torch.cuda.synchronize()
            calls[label] = _lib.CALLS - n0
            assert all(torch.isfinite(o).all() for o in out), label
            graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
            with torch.cuda.stream(side):
                with torch.cuda.graph(graph, stream=side):
                    gout = step(b)
            graph.replay(); torch.cuda.synchronize()
            if not torch.equal(gout[0], out[0]):
                print(f"{label}: graph replay differs from the eager forward by {float((gout[0] - out[0]).abs().max()):.3g}")
            runs[label] = (graph, gout, out)
        notes.append("encoder output with every clip on slot 0 " + ("equals" if torch.equal(runs["bank"][2][0], runs["no bank"][2][0]) else "DIFFERS from") +
                     " the bank-less encoder output, bit for bit")
        same = torch.equal(runs["bank"][2][1][:, :a.vocab].argmax(1), runs["no bank"][2][1].argmax(1))
        notes.append("greedy path of the bank's head on slot 0 " + ("equals" if same else "differs from") + " the linear decoder's (random weights: "
                     "near-ties may differ)")
        mixed = (torch.arange(a.batch, dtype=torch.int32) % a.slots).cuda()
        resident = torch.full((a.batch,), -1, dtype=torch.int32, device="cuda")
        for label, key, ids in (("no bank (first)", "no bank", None), ("bank, every clip on slot 0", "bank", resident),
                                (f"bank, {a.slots} languages, clip i on slot i mod {a.slots}", "bank", mixed), ("no bank (second)", "no bank", None)):
            if ids is not None:
                bank.ids[:a.batch].copy_(ids)
            run = runs[key][0].replay
            run(); run(); torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                run()
            torch.cuda.synchronize()
            res[label] = (time.perf_counter() - t0) / a.steps * 1e3
        moved = float((runs["bank"][1][0] - runs["no bank"][1][0]).abs().max())
        notes.append(f"max abs change of the encoder output under the mixed selection: {moved:.3g}")
    frames = out[0].shape[1]
    del runs, plan, bank, decoder
    torch.cuda.empty_cache()
    return res, frames, calls, notes


def time_launches(a, t, reps=50):
    """-> ({name: [us per block]}, {name: floor bytes}) at batch x t rows of 1280."""
    from thunder_speech_amd import _lib
    from thunder_speech_amd.blocks import linear_decoder
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    bf, b, slots, rows = torch.bfloat16, a.batch, a.slots, a.batch * t
    v_pad = -(-a.vocab // 16) * 16
    g = torch.Generator().manual_seed(4)
    h = torch.randn(b, t, C, generator=g).cuda()
    ones, zeros = torch.ones(slots, C).cuda(), torch.zeros(slots, C).cuda()
    w1, b1 = (torch.randn(slots, A, C, generator=g) / C ** 0.5).to(bf).cuda(), torch.zeros(slots, A).cuda()
    w2 = torch.zeros(slots, C, A, dtype=bf).cuda()                 # a zero term: the repeated in-place launches leave h as it is
    y16 = torch.empty(rows, C, dtype=bf, device="cuda")
    ids = (torch.arange(b, dtype=torch.int32) % slots).cuda()
    hw = (torch.randn(slots, v_pad, C, generator=g) / C ** 0.5).to(bf).cuda()
    hb = torch.zeros(slots, v_pad).cuda()
    vocab = torch.full((slots,), a.vocab, dtype=torch.int32, device="cuda")
    ldt = -(-t // 4) * 4
    logits = torch.empty(b, v_pad, ldt, device="cuda")
    decoder = linear_decoder(C, a.vocab, decoder_dropout=0.0).cuda().eval()
    hT = h.transpose(-1, -2)

    def run_decoder():
        with torch.no_grad():
            decoder(hT)
        return 0
    names = ("ts_mms_attn_adapter_fwd + LayerNorm (bf16 result)", "ts_mms_lang_bank_adapter_fwd + LayerNorm (bf16 result)",
             "linear decoder, eval forward (bf16 packing + TCS pointwise head)", "ts_mms_lang_bank_head_fwd")
    calls = {
        names[0]: lambda: L.ts_mms_attn_adapter_fwd(h.data_ptr(), rows, C, A, ones.data_ptr(), zeros.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
                                                    zeros.data_ptr(), ones.data_ptr(), zeros.data_ptr(), 1e-5, None, y16.data_ptr(), 1, s),
        names[1]: lambda: L.ts_mms_lang_bank_adapter_fwd(h.data_ptr(), b, t, C, A, ones.data_ptr(), zeros.data_ptr(), w1.data_ptr(), b1.data_ptr(),
                                                         w2.data_ptr(), zeros.data_ptr(), slots, ids.data_ptr(), ones.data_ptr(), zeros.data_ptr(), 1e-5,
                                                         None, y16.data_ptr(), 1, s),
        names[2]: run_decoder,
        names[3]: lambda: L.ts_mms_lang_bank_head_fwd(h.data_ptr(), b, t, C, hw.data_ptr(), hb.data_ptr(), vocab.data_ptr(), slots, v_pad, ids.data_ptr(),
                                                      logits.data_ptr(), ldt, 1, s),
    }
    pack = 2 * A * C * 2 + (3 * C + A) * 4                          # one slot's adapter tensors of one layer
    used = min(slots, b)
    floors = {names[0]: rows * C * (4 + 4 + 2) + pack, names[1]: rows * C * (4 + 4 + 2) + used * pack,
              names[2]: rows * C * 4 + b * a.vocab * t * 4 + a.vocab * C * 2,      # h once (f32), the logits, the weights; the bf16 copy not counted
              names[3]: rows * C * 4 + b * v_pad * t * 4 + used * v_pad * (C * 2 + 4)}
    times = _blocks(calls, reps)
    return times, floors


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seconds", type=int, default=20)
    ap.add_argument("--layers", type=int, default=48)
    ap.add_argument("--steps", type=int, default=20, help="timed graph replays per timing")
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--vocab", type=int, default=154, help="classes of the resident language (the bank pads to a multiple of 16)")
    ap.add_argument("--out", default=None, help="also write the tables (markdown) to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mms_lang_bank: needs an MI355X")
    box = torch.cuda.get_device_name(0)
    res, frames, calls, notes = time_steps(a)
    base = 0.5 * (res["no bank (first)"] + res["no bank (second)"])
    lines = [f"one process on one {box}; precision=\"bf16\", {a.batch} x {a.seconds} s, {a.layers} layers, 1280 hidden / 16 heads / 5120 FFN / adapter 16, random "
             f"weights, {frames} frames; step = waveform normalisation + encoder + CTC head ({a.vocab} classes; the bank pads to {-(-a.vocab // 16) * 16}); "
             f"graphed, 2 warm-up replays, then {a.steps} timed replays by the host clock, in the order of the table; both bank rows replay ONE graph", "",
             "| step | ms | vs mean of the two bank-less timings | C-ABI calls per step |", "|---|---:|---:|---:|"]
    for label, ms in res.items():
        lines.append(f"| {label} | {ms:.2f} | {ms / base:.4f} | {calls['no bank' if label.startswith('no bank') else 'bank']} |")
    lines += ["", f"spread of the two bank-less timings: {abs(res['no bank (first)'] - res['no bank (second)']):.2f} ms"] + [f"- {n}" for n in notes]
    times, floors = time_launches(a, frames)
    lines += ["", f"per launch: {a.batch} clips x {frames} frames = {a.batch * frames} rows x 1280, a = 16, {a.slots} slots, clip i on slot i mod {a.slots} (device events, "
              f"3 blocks of 50 launches, the four calls alternated); HBM floor at {HBM_PEAK / 1e12:.0f} TB/s from the shapes: adapter = rows x 1280 x (4 read + 4 "
              "written + 2 bf16 LayerNorm result) + the slots' tensors in use; head = h once in f32 + the logits + the heads in use:", "",
              "| launch | us per call (blocks) | best us | floor MB | HBM floor us | best / floor |", "|---|---|---:|---:|---:|---:|"]
    for k, us in times.items():
        fl = floors[k] / HBM_PEAK * 1e6
        lines.append(f"| {k} | {' / '.join(f'{v:.1f}' for v in us)} | {min(us):.1f} | {floors[k] / 1e6:.1f} | {fl:.1f} | {min(us) / fl:.2f} |")
    ks = list(times)
    d_ad, d_head = min(times[ks[1]]) - min(times[ks[0]]), min(times[ks[3]]) - min(times[ks[2]])
    lines += ["", f"by the per-call times the bank costs {a.layers} x {d_ad:.1f} us (adapter launches) + {d_head:.1f} us (head) = "
              f"{(a.layers * d_ad + d_head) / 1e3:.3f} ms per step; the mixed step above is {res[list(res)[2]] - base:.2f} ms from the bank-less mean"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
