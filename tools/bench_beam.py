"""Per-call device time of ts_ctc_beam_search (csrc/ctc_beam.hip: candidate pre-pass, search, backtrace) at bench_align.py's three shapes and the
settings (beam_width 16, token_cap 8) and (64, 16), and of ts_ctc_greedy_spans and the forward-only ts_ctc_loss on the same tensors in the same run.
python tools/bench_beam.py [--reps 20] [--out profiles/ctc_beam.md]

Logits: 2 x randn as bench_align.py ("flat": many classes of similar probability, the beam turns over at every frame), and the same with + 6 on the
blank and + 9 on one label in every fourth frame ("peaky": what a trained CTC model emits).  Random targets for the loss, every clip at full length.
Device events around `reps` back-to-back calls, the calls alternating, best of five blocks after a warm-up call of each."""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

SHAPES = [("wav2vec2: 16 x (T 999, S 150, V 32)", 16, 999, 150, 32),
          ("QuartzNet: 64 x (T 751, S 120, V 29)", 64, 751, 120, 29),
          ("long clip: 1 x (T 4999, S 700, V 32)", 1, 4999, 700, 32)]
SETTINGS = [(16, 8), (64, 16)]


def time_shape(L, b, t, s, v, peaky, reps, blocks=5):
    from thunder_speech_amd import _lib
    g = torch.Generator().manual_seed(b * 1000 + t)
    st = torch.cuda.current_stream().cuda_stream
    logits = 2 * torch.randn(b, v, t, generator=g)
    if peaky:
        logits[:, 0] += 6.0
        labels = torch.randint(1, v, (b, t), generator=g)
        hot = torch.zeros(b, v, t).scatter_(1, labels[:, None, :], 9.0)
        hot[:, :, torch.arange(t) % 4 != 0] = 0
        logits += hot
    logits = logits.cuda()
    targets = torch.randint(1, v, (b, s), generator=g, dtype=torch.int32).cuda()
    il = torch.full((b,), t, dtype=torch.int32, device="cuda")
    tl = torch.full((b,), s, dtype=torch.int32, device="cuda")
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device="cuda")
    f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device="cuda")
    g_tok, g_spans, g_logp, g_counts = i32(b, t), i32(b, t, 2), f32(b, t), i32(b)
    ws_g = torch.empty(L.ts_ctc_greedy_spans_workspace_bytes(b, t), dtype=torch.uint8, device="cuda")
    nll, loss = f32(b), f32(1)
    ws_l = torch.empty(L.ts_ctc_workspace_bytes(b, v, t, s), dtype=torch.uint8, device="cuda")
    calls = {
        "loss": lambda: L.ts_ctc_loss(logits.data_ptr(), b, v, t, t, targets.data_ptr(), s, il.data_ptr(), tl.data_ptr(), 0, nll.data_ptr(),
                                      loss.data_ptr(), None, ws_l.data_ptr(), st),
        "greedy": lambda: L.ts_ctc_greedy_spans(logits.data_ptr(), b, v, t, t, None, 0, g_tok.data_ptr(), g_spans.data_ptr(), g_logp.data_ptr(),
                                                g_counts.data_ptr(), ws_g.data_ptr(), st),
    }
    keep, cfgs = [], {}
    for width, cap in SETTINGS:
        n_best = min(width, 4)
        out = [i32(b, n_best, t), i32(b, n_best, t), i32(b, n_best), f32(b, n_best), i32(b)]
        ws = torch.empty(L.ts_ctc_beam_workspace_bytes(b, t, width, cap), dtype=torch.uint8, device="cuda")
        keep.append((out, ws))
        cfg = [C.c_int32(0) for _ in range(3)]
        _lib.check(L.ts_ctc_beam_launch_config(v, width, cap, *[C.addressof(c) for c in cfg]), "ts_ctc_beam_launch_config")
        cfgs[(width, cap)] = tuple(c.value for c in cfg)
        calls[(width, cap)] = (lambda width=width, cap=cap, n_best=n_best, out=out, ws=ws: L.ts_ctc_beam_search(
            logits.data_ptr(), b, v, t, t, None, 0, width, cap, n_best, *[o.data_ptr() for o in out], ws.data_ptr(), st))
    best = {name: float("inf") for name in calls}
    for name, f in calls.items():
        _lib.check(f(), str(name))
    torch.cuda.synchronize()
    for _ in range(blocks):
        for name, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            best[name] = min(best[name], e0.elapsed_time(e1) / reps * 1e3)
    produced = {k: int(keep[i][0][4].min()) for i, k in enumerate(SETTINGS)}
    return best, cfgs, produced


def main():
    ap = argparse.ArgumentParser(description="ts_ctc_beam_search per call, next to ts_ctc_greedy_spans and the forward-only ts_ctc_loss on the same tensors")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the table (markdown) to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_beam: needs an MI355X")
    from thunder_speech_amd import _lib
    L = _lib.lib()
    lines = [f"Device events around {a.reps} back-to-back calls, the calls alternating, best of 5 blocks after a warm-up call of each; flat = 2 x randn logits, "
             "peaky = the same with + 6 on the blank and + 9 on one label in every fourth frame; every clip at full length, n_best 4.", "",
             "| shape | logits | beam_width, token_cap | ranked candidates, threads | ts_ctc_beam_search us | per frame ns | ts_ctc_loss forward only us | beam / loss | "
             "ts_ctc_greedy_spans us | beam / greedy |", "|---|---|---|---|---:|---:|---:|---:|---:|---:|"]
    for name, b, t, s, v in SHAPES:
        for peaky in (False, True):
            best, cfgs, produced = time_shape(L, b, t, s, v, peaky, a.reps)
            for width, cap in SETTINGS:
                threads, _, cands = cfgs[(width, cap)]
                bm, lo, gr = best[(width, cap)], best["loss"], best["greedy"]
                lines.append(f"| {name} | {'peaky' if peaky else 'flat'} | {width}, {cap} | {cands}, {threads} | {bm:.1f} | {bm / t * 1e3:.0f} | {lo:.1f} | {bm / lo:.2f} | "
                             f"{gr:.1f} | {bm / gr:.1f} |")
                if produced[(width, cap)] < min(width, 4):
                    lines.append(f"| (a clip produced only {produced[(width, cap)]} hypotheses) | | | | | | | | | |")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
