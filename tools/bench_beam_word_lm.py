"""Per-call device time of ts_ctc_beam_word_lm_search (csrc/ctc_beam_word_lm.hip: candidate pre-pass, word-level fused search, backtrace) next to
ts_ctc_beam_lm_search and ts_ctc_beam_search on the same tensors in the same run, at bench_beam_lm.py's shapes and its two settings.
python tools/bench_beam_word_lm.py [--reps 10] [--out profiles/ctc_beam_word_lm.md]

Class 0 is the blank, class 1 the word delimiter, the others letters.  The word LM: a synthetic random order-3 table over a lexicon of 10000 random
spellings of 3 to 8 letters (every word a unigram, 20000 bigrams and 20000 trigrams, three quarters of their words from 300 common ones), 20 hot
words, alpha 0.5, beta 1.0, oov_score -4, hotword_weight 2, </s> scored.  Logits: every clip is a sequence of words of 3 to 8 letters, four in five
from the lexicon, a letter every fourth frame and a delimiter after each word; "peaky" puts + 9 on that label and + 6 on the blank as
bench_beam.py does, "flat" is 2 x randn with + 3 on the delimiter in the delimiter's frames only (- 3 elsewhere), so that words stay 3 to 8 letters
long.  The token-level LM of the middle column is bench_beam_lm.py's.  Device events around `reps` back-to-back calls, the calls alternating, best
of five blocks after a warm-up call of each."""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from bench_beam import SHAPES
from bench_beam_lm import ALPHA, BETA, SETTINGS, random_lm

ORDER, N_WORDS, OOV, HOT = 3, 10000, -4.0, 2.0
DELIM = 1


def itos_of(v):
    return ["<blank>", " "] + [chr(0x61 + i) if i < 26 else chr(0x100 + i) for i in range(v - 2)]


def random_word_lm(v, seed=0):
    from thunder_speech_amd.ctc_lm import WordNGramLM
    rng = np.random.Generator(np.random.PCG64(seed))
    itos = itos_of(v)
    words = set()
    while len(words) < N_WORDS:
        words.add("".join(itos[int(c)] for c in rng.integers(2, v, int(rng.integers(3, 9)))))
    words = sorted(words)
    common = [words[int(i)] for i in rng.permutation(N_WORDS)[:300]]
    pick = lambda: common[int(rng.integers(300))] if rng.random() < 0.75 else words[int(rng.integers(N_WORDS))]
    val = lambda n: (float(rng.uniform(-4.0, -0.5)), float(rng.uniform(-1.0, 0.0)) if n < ORDER else 0.0)
    grams = {("<s>",): (-99.0, -0.3), ("</s>",): val(ORDER), ("<unk>",): val(ORDER)}
    for w in words:
        grams[(w,)] = val(1)
    for n in (2, 3):
        for _ in range(20000):
            g = tuple(pick() for _ in range(n))
            grams[g] = val(n)
            if rng.random() < 0.1:
                grams[("<s>",) + g[1:]] = val(n)
            if rng.random() < 0.1:
                grams[g[:-1] + ("</s>",)] = (val(n)[0], 0.0)
    return WordNGramLM(ORDER, grams, itos, 0, " ", None, common[:20]), words


def word_logits(b, t, v, peaky, words, seed):
    """[b, v, t] logits of clips that say words: a label every fourth frame, the delimiter after each word."""
    rng = np.random.Generator(np.random.PCG64(seed))
    itos = itos_of(v)
    labels = np.zeros((b, t), np.int64)
    for i in range(b):
        seq = []
        while len(seq) < (t + 3) // 4:
            w = words[int(rng.integers(len(words)))] if rng.random() < 0.8 else "".join(itos[int(c)] for c in rng.integers(2, v, int(rng.integers(3, 9))))
            seq += [itos.index(ch) for ch in w] + [DELIM]
        labels[i, ::4] = seq[: (t + 3) // 4]
    g = torch.Generator().manual_seed(seed)
    logits = 2 * torch.randn(b, v, t, generator=g)
    lab = torch.from_numpy(labels)
    if peaky:
        logits[:, 0] += 6.0
        hot = torch.zeros(b, v, t).scatter_(1, lab[:, None, :], 9.0)
        hot[:, :, torch.arange(t) % 4 != 0] = 0
        logits += hot
    else:
        logits[:, DELIM] += torch.where(lab == DELIM, 3.0, -3.0)
    return logits


def time_shape(L, lm, words, tok_lm, b, t, v, peaky, reps, blocks=5):
    from thunder_speech_amd import _lib
    st = torch.cuda.current_stream().cuda_stream
    logits = word_logits(b, t, v, peaky, words, b * 1000 + t).cuda()
    w, wt = lm.weights(ALPHA, BETA, OOV, HOT), tok_lm.weights(ALPHA, BETA)
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device="cuda")
    f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device="cuda")
    calls, keep, cfgs = {}, [], {}
    for width, cap in SETTINGS:
        n_best = min(width, 4)
        plain_out = [i32(b, n_best, t), i32(b, n_best, t), i32(b, n_best), f32(b, n_best), i32(b)]
        fused_out = lambda: [i32(b, n_best, t), i32(b, n_best, t), i32(b, n_best), f32(b, n_best), f32(b, n_best), i32(b)]
        out_lm, out_word = fused_out(), fused_out()
        ws = torch.empty(L.ts_ctc_beam_workspace_bytes(b, t, width, cap), dtype=torch.uint8, device="cuda")
        ws_lm = torch.empty(L.ts_ctc_beam_lm_workspace_bytes(b, t, width, cap), dtype=torch.uint8, device="cuda")
        ws_word = torch.empty(L.ts_ctc_beam_word_lm_workspace_bytes(b, t, width, cap), dtype=torch.uint8, device="cuda")
        keep.append((plain_out, out_lm, out_word, ws, ws_lm, ws_word))
        cfg = [C.c_int32(0) for _ in range(3)]
        _lib.check(L.ts_ctc_beam_word_lm_launch_config(v, width, cap, *[C.addressof(c) for c in cfg]), "word launch config")
        cfgs[(width, cap)] = tuple(c.value for c in cfg)
        calls[("plain", width, cap)] = (lambda width=width, cap=cap, n_best=n_best, out=plain_out, ws=ws: L.ts_ctc_beam_search(
            logits.data_ptr(), b, v, t, t, None, 0, width, cap, n_best, *[o.data_ptr() for o in out], ws.data_ptr(), st))
        calls[("lm", width, cap)] = (lambda width=width, cap=cap, n_best=n_best, out=out_lm, ws=ws_lm: L.ts_ctc_beam_lm_search(
            logits.data_ptr(), b, v, t, t, None, 0, width, cap, n_best, 1, C.byref(wt.struct), *[o.data_ptr() for o in out], ws.data_ptr(), st))
        calls[("word", width, cap)] = (lambda width=width, cap=cap, n_best=n_best, out=out_word, ws=ws_word: L.ts_ctc_beam_word_lm_search(
            logits.data_ptr(), b, v, t, t, None, 0, width, cap, n_best, 1, C.byref(w.lm.struct), C.byref(w.struct), *[o.data_ptr() for o in out],
            ws.data_ptr(), st))
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
    # what the best hypotheses look like: words per clip and how many of them the lexicon holds
    tokens, lengths = keep[0][2][0][:, 0].cpu().numpy(), keep[0][2][2][:, 0].cpu().numpy()
    n_words = n_in = 0
    for i in range(b):
        text = "".join(itos_of(v)[c] for c in tokens[i, : lengths[i]])
        found = [x for x in text.split(" ") if x]
        n_words, n_in = n_words + len(found), n_in + sum(x in lm.words for x in found)
    return best, cfgs, (n_words / b, n_in / max(n_words, 1))


def main():
    ap = argparse.ArgumentParser(description="ts_ctc_beam_word_lm_search per call, next to ts_ctc_beam_lm_search and ts_ctc_beam_search on the same tensors")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the table (markdown) to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_beam_word_lm: needs an MI355X")
    from thunder_speech_amd import _lib
    L = _lib.lib()
    lms = {}
    lines = [f"Device events around {a.reps} back-to-back calls, the calls alternating, best of 5 blocks after a warm-up call of each; every clip says words of 3 to 8 "
             "letters (four in five from the lexicon), a letter every fourth frame, a delimiter after each word; peaky = 2 x randn with + 6 on the blank and + 9 on "
             "that label, flat = 2 x randn with + 3 on the delimiter in its frames and - 3 elsewhere; every clip at full length, n_best 4.  Word LM: synthetic "
             f"random order-{ORDER} table over {N_WORDS} random spellings, 20 hot words, alpha {ALPHA}, beta {BETA}, oov_score {OOV}, hotword_weight {HOT}, </s> "
             "scored; token LM: that of tools/bench_beam_lm.py.", "",
             "| shape | logits | beam_width, token_cap | candidates, threads | ts_ctc_beam_word_lm_search us | per frame ns | ts_ctc_beam_lm_search us | "
             "ts_ctc_beam_search us | word / token LM | word / plain | words per clip (16, 8), in lexicon |", "|---|---|---|---|---:|---:|---:|---:|---:|---:|---|"]
    sizes = []
    for name, b, t, _, v in SHAPES:
        if v not in lms:
            lms[v] = random_word_lm(v) + (random_lm(v, 0),)
            lm = lms[v][0]
            sizes.append(f"V = {v}: word automaton {lm.lm.n_states} states, {sum(len(x) for x in lm.lm.arcs)} arcs; trie {lm.n_nodes} nodes, {len(lm.words)} words")
        lm, words, tok_lm = lms[v]
        for peaky in (False, True):
            best, cfgs, (per_clip, share) = time_shape(L, lm, words, tok_lm, b, t, v, peaky, a.reps)
            for width, cap in SETTINGS:
                threads, _, cands = cfgs[(width, cap)]
                word, tok, plain = best[("word", width, cap)], best[("lm", width, cap)], best[("plain", width, cap)]
                lines.append(f"| {name} | {'peaky' if peaky else 'flat'} | {width}, {cap} | {cands}, {threads} | {word:.1f} | {word / t * 1e3:.0f} | {tok:.1f} | "
                             f"{plain:.1f} | {word / tok:.2f} | {word / plain:.2f} | {per_clip:.0f}, {share:.0%} |")
    lines += ["", "Tables: " + "; ".join(sizes) + "."]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
