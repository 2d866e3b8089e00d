"""Per-call device time of ts_ctc_align and ts_ctc_greedy_spans (csrc/ctc_align.hip) at three shapes, and of the forward-only ts_ctc_loss
(csrc/ctc.hip, grad = NULL: one workgroup per utterance, the same serial skeleton with three exponentials and a logarithm more per step) on the
same tensors in the same run.
python tools/bench_align.py [--reps 50] [--out profiles/ctc_align.md]

Random logits (2 x randn), random targets, every clip at full length.  Device events around `reps` back-to-back calls, the three calls alternating,
best of five blocks after a warm-up call of each."""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

SHAPES = [("wav2vec2: 16 x (T 999, S 150, V 32)", 16, 999, 150, 32),
          ("QuartzNet: 64 x (T 751, S 120, V 29)", 64, 751, 120, 29),
          ("long clip: 1 x (T 4999, S 700, V 32)", 1, 4999, 700, 32)]


def time_shape(L, b, t, s, v, reps, blocks=5):
    from thunder_speech_amd import _lib
    g = torch.Generator().manual_seed(b * 1000 + t)
    st = torch.cuda.current_stream().cuda_stream
    logits = (2 * torch.randn(b, v, t, generator=g)).cuda()
    targets = torch.randint(1, v, (b, s), generator=g, dtype=torch.int32).cuda()
    il = torch.full((b,), t, dtype=torch.int32, device="cuda")
    tl = torch.full((b,), s, dtype=torch.int32, device="cuda")
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device="cuda")
    f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device="cuda")
    path, spans, logp, score = i32(b, t), i32(b, s, 2), f32(b, s), f32(b)
    ws_a = torch.empty(L.ts_ctc_align_workspace_bytes(b, t, s), dtype=torch.uint8, device="cuda")
    g_tok, g_spans, g_logp, g_counts = i32(b, t), i32(b, t, 2), f32(b, t), i32(b)
    ws_g = torch.empty(L.ts_ctc_greedy_spans_workspace_bytes(b, t), dtype=torch.uint8, device="cuda")
    nll, loss = f32(b), f32(1)
    ws_l = torch.empty(L.ts_ctc_workspace_bytes(b, v, t, s), dtype=torch.uint8, device="cuda")
    cfg = [C.c_int32(0) for _ in range(4)]
    _lib.check(L.ts_ctc_align_launch_config(t, s, *[C.addressof(c) for c in cfg]), "ts_ctc_align_launch_config")
    calls = {
        "ts_ctc_align": lambda: L.ts_ctc_align(logits.data_ptr(), b, v, t, t, targets.data_ptr(), s, il.data_ptr(), tl.data_ptr(), 0, path.data_ptr(),
                                               spans.data_ptr(), logp.data_ptr(), score.data_ptr(), ws_a.data_ptr(), st),
        "ts_ctc_loss forward only": lambda: L.ts_ctc_loss(logits.data_ptr(), b, v, t, t, targets.data_ptr(), s, il.data_ptr(), tl.data_ptr(), 0,
                                                          nll.data_ptr(), loss.data_ptr(), None, ws_l.data_ptr(), st),
        "ts_ctc_greedy_spans": lambda: L.ts_ctc_greedy_spans(logits.data_ptr(), b, v, t, t, None, 0, g_tok.data_ptr(), g_spans.data_ptr(), g_logp.data_ptr(),
                                                             g_counts.data_ptr(), ws_g.data_ptr(), st),
    }
    best = {name: float("inf") for name in calls}
    for name, f in calls.items():
        _lib.check(f(), name)
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
    feasible = int(torch.isfinite(score).sum())
    return best, tuple(c.value for c in cfg), feasible


def main():
    ap = argparse.ArgumentParser(description="ts_ctc_align / ts_ctc_greedy_spans per call, next to the forward-only ts_ctc_loss on the same tensors")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None, help="also write the table (markdown) to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_align: needs an MI355X")
    from thunder_speech_amd import _lib
    L = _lib.lib()
    lines = [f"Device events around {a.reps} back-to-back calls, the three calls alternating, best of 5 blocks after a warm-up call of each; 2 x randn logits, "
             "random targets, every clip at full length.", "",
             "| shape | states per thread, threads, back-pointers | ts_ctc_align us | ts_ctc_loss forward only us | align / loss | per frame ns (align) | "
             "ts_ctc_greedy_spans us |", "|---|---|---:|---:|---:|---:|---:|"]
    for name, b, t, s, v in SHAPES:
        best, (spt, threads, bp_lds, lds), feasible = time_shape(L, b, t, s, v, a.reps)
        al, lo, gr = best["ts_ctc_align"], best["ts_ctc_loss forward only"], best["ts_ctc_greedy_spans"]
        where = f"LDS ({lds / 1024:.0f} KiB)" if bp_lds else "workspace"
        lines.append(f"| {name} | {spt}, {threads}, {where} | {al:.1f} | {lo:.1f} | {al / lo:.2f} | {al / t * 1e3:.0f} | {gr:.1f} |")
        if feasible != b:
            lines.append(f"| ({b - feasible} of {b} clips infeasible) | | | | | | |")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
