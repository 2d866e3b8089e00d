"""Per-call device time of ts_ctc_beam_lm_search (csrc/ctc_beam_lm.hip: candidate pre-pass, fused search, backtrace) next to ts_ctc_beam_search on the
same tensors in the same run, at bench_beam.py's three shapes and the settings (beam_width 16, token_cap 8) and (64, 15) -- the second is the
fused search's limit of 1024 candidates.
python tools/bench_beam_lm.py [--reps 10] [--out profiles/ctc_beam_lm.md]

Logits as bench_beam.py ("flat" and "peaky").  The LM: a random order-5 n-gram table over V = 32 (about half of the unigrams and bigrams, 3000
n-grams of each longer order, three quarters of their words from eight classes, so that the search meets them), alpha 0.5, beta 1.0, </s> scored.
Device events around `reps` back-to-back calls, the calls alternating, best of five blocks after a warm-up call of each."""
import argparse
import ctypes as C
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench_beam import SHAPES

SETTINGS = [(16, 8), (64, 15)]
ORDER, ALPHA, BETA = 5, 0.5, 1.0


def random_lm(v, blank, seed=0):
    from thunder_speech_amd.ctc_lm import BOS, EOS, UNK, NGramLM
    rng = np.random.Generator(np.random.PCG64(seed))
    words = [c for c in range(v) if c != blank]
    common = words[:8]
    val = lambda n: (float(rng.uniform(-3.0, -0.1)), float(rng.uniform(-1.0, 0.0)) if n < ORDER else 0.0)
    grams = {(BOS,): (-99.0, -0.3), (EOS,): val(ORDER), (UNK,): val(ORDER)}
    for n in (1, 2):
        for g in itertools.product(words, repeat=n):
            if rng.random() < 0.5:
                grams[g] = val(n)
    for n in range(3, ORDER + 1):
        for _ in range(3000):
            g = tuple(int(rng.choice(common)) if rng.random() < 0.75 else int(rng.choice(words)) for _ in range(n))
            grams[g] = val(n)
            if rng.random() < 0.1:
                grams[(BOS,) + g[1:]] = val(n)
            if rng.random() < 0.1:
                grams[g[:-1] + (EOS,)] = (val(n)[0], 0.0)
    return NGramLM(ORDER, grams, v, blank)


def time_shape(L, lm, b, t, v, peaky, reps, blocks=5):
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
    w = lm.weights(ALPHA, BETA)
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device="cuda")
    f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device="cuda")
    calls, keep, cfgs = {}, [], {}
    for width, cap in SETTINGS:
        n_best = min(width, 4)
        out = [i32(b, n_best, t), i32(b, n_best, t), i32(b, n_best), f32(b, n_best), i32(b)]
        ws = torch.empty(L.ts_ctc_beam_workspace_bytes(b, t, width, cap), dtype=torch.uint8, device="cuda")
        out_lm = [i32(b, n_best, t), i32(b, n_best, t), i32(b, n_best), f32(b, n_best), f32(b, n_best), i32(b)]
        ws_lm = torch.empty(L.ts_ctc_beam_lm_workspace_bytes(b, t, width, cap), dtype=torch.uint8, device="cuda")
        keep.append((out, ws, out_lm, ws_lm))
        for name, fn in (("plain", L.ts_ctc_beam_launch_config), ("lm", L.ts_ctc_beam_lm_launch_config)):
            cfg = [C.c_int32(0) for _ in range(3)]
            _lib.check(fn(v, width, cap, *[C.addressof(c) for c in cfg]), name + " launch config")
            cfgs[(name, width, cap)] = tuple(c.value for c in cfg)
        calls[("plain", width, cap)] = (lambda width=width, cap=cap, n_best=n_best, out=out, ws=ws: L.ts_ctc_beam_search(
            logits.data_ptr(), b, v, t, t, None, 0, width, cap, n_best, *[o.data_ptr() for o in out], ws.data_ptr(), st))
        calls[("lm", width, cap)] = (lambda width=width, cap=cap, n_best=n_best, out=out_lm, ws=ws_lm: L.ts_ctc_beam_lm_search(
            logits.data_ptr(), b, v, t, t, None, 0, width, cap, n_best, 1, C.byref(w.struct), *[o.data_ptr() for o in out], ws.data_ptr(), st))
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
    return best, cfgs


def main():
    ap = argparse.ArgumentParser(description="ts_ctc_beam_lm_search per call, next to ts_ctc_beam_search on the same tensors")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the table (markdown) to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_beam_lm: needs an MI355X")
    from thunder_speech_amd import _lib
    L = _lib.lib()
    lm = random_lm(32, 0)
    lines = [f"Device events around {a.reps} back-to-back calls, the calls alternating, best of 5 blocks after a warm-up call of each; flat = 2 x randn logits, "
             "peaky = the same with + 6 on the blank and + 9 on one label in every fourth frame; every clip at full length, n_best 4.  LM: random order-5 "
             f"table over V = 32 ({lm.n_states} states, {sum(len(x) for x in lm.arcs)} arcs), alpha {ALPHA}, beta {BETA}, </s> scored.", "",
             "| shape | logits | beam_width, token_cap | fused: candidates, threads | ts_ctc_beam_lm_search us | per frame ns | plain: candidates, threads | "
             "ts_ctc_beam_search us | fused / plain |", "|---|---|---|---|---:|---:|---|---:|---:|"]
    for name, b, t, _, v in SHAPES:
        for peaky in (False, True):
            best, cfgs = time_shape(L, lm, b, t, v, peaky, a.reps)
            for width, cap in SETTINGS:
                (pt, _, pc), (lt, _, lc) = cfgs[("plain", width, cap)], cfgs[("lm", width, cap)]
                fused, plain = best[("lm", width, cap)], best[("plain", width, cap)]
                lines.append(f"| {name} | {'peaky' if peaky else 'flat'} | {width}, {cap} | {lc}, {lt} | {fused:.1f} | {fused / t * 1e3:.0f} | {pc}, {pt} | {plain:.1f} | "
                             f"{fused / plain:.2f} |")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
