"""Per-call device time of ts_ctc_beam_piece_lm_search (csrc/ctc_beam_piece_lm.hip: candidate pre-pass, word-level fused search over pieces,
backtrace) next to ts_ctc_beam_lm_search (the token-level LM over the same pieces) and ts_ctc_beam_search on the same tensors in the same run, at
Citrinet's shapes -- 8x downsampling of 20 s and 15 s clips, 1024 pieces and the blank -- and the settings (beam_width 16, token_cap 8) and (64, 15).
python tools/bench_beam_piece_lm.py [--reps 10] [--out profiles/ctc_beam_piece_lm.md]

The word LM: a synthetic random order-3 table over a lexicon of 10000 random spellings of 3 to 8 letters (every word a unigram, 20000 bigrams and
20000 trigrams, three quarters of their words from 300 common ones), 20 hot words, alpha 0.5, beta 1.0, oov_score -4, hotword_weight 2, </s> scored.
The piece inventory: the bare word start, the 26 letters with and without the word start, and the most frequent beginnings (with the word start)
and inner stretches (without) of 2 to 4 letters of the lexicon's words, common words counted 30 times, up to 1024 pieces; the blank is the last
class, as in a Citrinet vocabulary.  The token-level LM of the middle column: a random order-3 table over the pieces (every piece a unigram, 20000
bigrams and 20000 trigrams).  Logits: every clip is a sequence of words, four in five from the lexicon, cut into pieces by longest match, a piece
every other frame; "peaky" puts + 9 on that piece and + 6 on the blank, "flat" is 2 x randn with + 4 on that piece.  Device events around `reps`
back-to-back calls, the calls alternating, best of five blocks after a warm-up call of each."""
import argparse
import collections
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

SHAPES = [("16 x 20 s", 16, 250, 1025), ("64 x 15 s", 64, 188, 1025)]          # name, clips, frames, classes
SETTINGS = [(16, 8), (64, 15)]
ORDER, N_WORDS, ALPHA, BETA, OOV, HOT = 3, 10000, 0.5, 1.0, -4.0, 2.0
WS = "▁"
LETTERS = [chr(0x61 + i) for i in range(26)]


def random_words(seed=0):
    """(the lexicon's words, sorted; the 300 common ones)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    words = set()
    while len(words) < N_WORDS:
        words.add("".join(LETTERS[int(c)] for c in rng.integers(0, 26, int(rng.integers(3, 9)))))
    words = sorted(words)
    return words, [words[int(i)] for i in rng.permutation(N_WORDS)[:300]]


def piece_inventory(words, common, v):
    """itos of v classes: the pieces by frequency, the blank last."""
    weight = collections.Counter({w: 1 for w in words})
    weight.update({w: 29 for w in common})
    count = collections.Counter()
    for w, n in weight.items():
        for k in range(2, min(len(w), 4) + 1):
            count[WS + w[:k]] += n
            for j in range(1, len(w) - k + 1):
                count[w[j:j + k]] += n
    base = [WS] + [WS + ch for ch in LETTERS] + LETTERS
    multi = [p for p, _ in sorted(count.items(), key=lambda kv: (-kv[1], kv[0]))[: v - 1 - len(base)]]
    return base + multi + ["<blank>"]


def segment(word, pieces):
    """`word` in pieces by longest match: a piece that starts a word, then pieces that continue it."""
    out, rest, first = [], word, True
    while rest or first:
        for k in range(min(len(rest), 4), -1, -1):
            p = (WS if first else "") + rest[:k]
            if p in pieces and (k > 0 or first):
                out.append(p)
                rest, first = rest[k:], False
                break
    return out


def random_word_lm(itos, words, common, seed=1):
    from thunder_speech_amd.ctc_lm import PieceWordNGramLM
    rng = np.random.Generator(np.random.PCG64(seed))
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
    return PieceWordNGramLM(ORDER, grams, itos, len(itos) - 1, WS, None, common[:20])


def random_piece_lm(v, seed=2):
    """The token-level LM over the same classes: every piece a unigram, 20000 bigrams and trigrams, three quarters of their pieces from 100."""
    from thunder_speech_amd.ctc_lm import BOS, EOS, UNK, NGramLM
    rng = np.random.Generator(np.random.PCG64(seed))
    pick = lambda: int(rng.integers(100)) if rng.random() < 0.75 else int(rng.integers(v - 1))
    val = lambda n: (float(rng.uniform(-4.0, -0.5)), float(rng.uniform(-1.0, 0.0)) if n < ORDER else 0.0)
    grams = {(BOS,): (-99.0, -0.3), (EOS,): val(ORDER), (UNK,): val(ORDER)}
    for c in range(v - 1):
        grams[(c,)] = val(1)
    for n in (2, 3):
        for _ in range(20000):
            g = tuple(pick() for _ in range(n))
            grams[g] = val(n)
            if rng.random() < 0.1:
                grams[(BOS,) + g[1:]] = val(n)
            if rng.random() < 0.1:
                grams[g[:-1] + (EOS,)] = (val(n)[0], 0.0)
    return NGramLM(ORDER, grams, v, v - 1)


def piece_logits(b, t, itos, peaky, words, seed):
    """[b, v, t] logits of clips that say words in pieces: a piece every other frame."""
    rng = np.random.Generator(np.random.PCG64(seed))
    v, blank, pieces, where = len(itos), len(itos) - 1, set(itos), {p: c for c, p in enumerate(itos)}
    labels = np.full((b, t), blank, np.int64)
    for i in range(b):
        seq = []
        while len(seq) < (t + 1) // 2:
            w = words[int(rng.integers(len(words)))] if rng.random() < 0.8 else "".join(LETTERS[int(c)] for c in rng.integers(0, 26, int(rng.integers(3, 9))))
            seq += [where[p] for p in segment(w, pieces)]
        labels[i, ::2] = seq[: (t + 1) // 2]
    g = torch.Generator().manual_seed(seed)
    logits = 2 * torch.randn(b, v, t, generator=g)
    said = torch.zeros(b, v, t).scatter_(1, torch.from_numpy(labels)[:, None, :], 1.0)
    said[:, blank] = 0
    if peaky:
        logits[:, blank] += 6.0
    return logits + (9.0 if peaky else 4.0) * said


def time_shape(L, lm, tok_lm, itos, words, b, t, peaky, reps, blocks=5):
    from thunder_speech_amd import _lib
    st = torch.cuda.current_stream().cuda_stream
    v, blank = len(itos), len(itos) - 1
    logits = piece_logits(b, t, itos, peaky, words, b * 1000 + t).cuda()
    w, wt = lm.weights(ALPHA, BETA, OOV, HOT), tok_lm.weights(ALPHA, BETA)
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device="cuda")
    f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device="cuda")
    calls, keep, cfgs = {}, [], {}
    for width, cap in SETTINGS:
        n_best = min(width, 4)
        plain_out = [i32(b, n_best, t), i32(b, n_best, t), i32(b, n_best), f32(b, n_best), i32(b)]
        fused_out = lambda: [i32(b, n_best, t), i32(b, n_best, t), i32(b, n_best), f32(b, n_best), f32(b, n_best), i32(b)]
        out_lm, out_piece = fused_out(), fused_out()
        ws = torch.empty(L.ts_ctc_beam_workspace_bytes(b, t, width, cap), dtype=torch.uint8, device="cuda")
        ws_lm = torch.empty(L.ts_ctc_beam_lm_workspace_bytes(b, t, width, cap), dtype=torch.uint8, device="cuda")
        ws_piece = torch.empty(L.ts_ctc_beam_piece_lm_workspace_bytes(b, t, width, cap), dtype=torch.uint8, device="cuda")
        keep.append((plain_out, out_lm, out_piece, ws, ws_lm, ws_piece))
        cfg = [C.c_int32(0) for _ in range(3)]
        _lib.check(L.ts_ctc_beam_piece_lm_launch_config(v, width, cap, *[C.addressof(c) for c in cfg]), "piece launch config")
        cfgs[(width, cap)] = tuple(c.value for c in cfg)
        calls[("plain", width, cap)] = (lambda width=width, cap=cap, n_best=n_best, out=plain_out, ws=ws: L.ts_ctc_beam_search(
            logits.data_ptr(), b, v, t, t, None, blank, width, cap, n_best, *[o.data_ptr() for o in out], ws.data_ptr(), st))
        calls[("lm", width, cap)] = (lambda width=width, cap=cap, n_best=n_best, out=out_lm, ws=ws_lm: L.ts_ctc_beam_lm_search(
            logits.data_ptr(), b, v, t, t, None, blank, width, cap, n_best, 1, C.byref(wt.struct), *[o.data_ptr() for o in out], ws.data_ptr(), st))
        calls[("piece", width, cap)] = (lambda width=width, cap=cap, n_best=n_best, out=out_piece, ws=ws_piece: L.ts_ctc_beam_piece_lm_search(
            logits.data_ptr(), b, v, t, t, None, blank, width, cap, n_best, 1, C.byref(w.lm.struct), C.byref(w.struct), C.byref(w.pieces),
            *[o.data_ptr() for o in out], ws.data_ptr(), st))
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
    n_words = n_in = n_pieces = 0
    for i in range(b):
        found = [x for x in "".join(itos[c] for c in tokens[i, : lengths[i]]).replace(WS, " ").split(" ") if x]
        n_words, n_in, n_pieces = n_words + len(found), n_in + sum(x in lm.words for x in found), n_pieces + int(lengths[i])
    return best, cfgs, (n_words / b, n_in / max(n_words, 1), n_pieces / max(n_words, 1))


def main():
    ap = argparse.ArgumentParser(description="ts_ctc_beam_piece_lm_search per call, next to ts_ctc_beam_lm_search and ts_ctc_beam_search on the same tensors")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the table (markdown) to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_beam_piece_lm: needs an MI355X")
    from thunder_speech_amd import _lib
    L = _lib.lib()
    words, common = random_words()
    lines = [f"Device events around {a.reps} back-to-back calls, the calls alternating, best of 5 blocks after a warm-up call of each; every clip says words of 3 to 8 "
             "letters (four in five from the lexicon) cut into pieces by longest match, a piece every other frame; peaky = 2 x randn with + 6 on the blank and + 9 "
             "on that piece, flat = 2 x randn with + 4 on that piece; every clip at full length, n_best 4.  Word LM: synthetic random "
             f"order-{ORDER} table over {N_WORDS} random spellings, 20 hot words, alpha {ALPHA}, beta {BETA}, oov_score {OOV}, hotword_weight {HOT}, </s> scored; "
             f"token LM: random order-{ORDER} table over the same pieces.", "",
             "| shape | logits | beam_width, token_cap | candidates, threads | ts_ctc_beam_piece_lm_search us | per frame ns | ts_ctc_beam_lm_search us | "
             "ts_ctc_beam_search us | piece / token LM | piece / plain | words per clip (16, 8), in lexicon, pieces per word |",
             "|---|---|---|---|---:|---:|---:|---:|---:|---:|---|"]
    lms, sizes = {}, []
    for name, b, t, v in SHAPES:
        if v not in lms:
            itos = piece_inventory(words, common, v)
            lms[v] = (itos, random_word_lm(itos, words, common), random_piece_lm(v))
            lm = lms[v][1]
            sizes.append(f"V = {v}: word automaton {lm.lm.n_states} states, {sum(len(x) for x in lm.lm.arcs)} arcs; trie {lm.n_nodes} nodes, {len(lm.words)} words; "
                         f"{len(lm.letters)} letters, {sum(len(p) for p in lm.piece_letters)} piece letters")
        itos, lm, tok_lm = lms[v]
        for peaky in (False, True):
            best, cfgs, (per_clip, share, per_word) = time_shape(L, lm, tok_lm, itos, words, b, t, peaky, a.reps)
            for width, cap in SETTINGS:
                threads, _, cands = cfgs[(width, cap)]
                piece, tok, plain = best[("piece", width, cap)], best[("lm", width, cap)], best[("plain", width, cap)]
                lines.append(f"| {name} (T {t}, V {v}) | {'peaky' if peaky else 'flat'} | {width}, {cap} | {cands}, {threads} | {piece:.1f} | {piece / t * 1e3:.0f} | "
                             f"{tok:.1f} | {plain:.1f} | {piece / tok:.2f} | {piece / plain:.2f} | {per_clip:.0f}, {share:.0%}, {per_word:.1f} |")
    lines += ["", "Tables: " + "; ".join(sizes) + "."]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
