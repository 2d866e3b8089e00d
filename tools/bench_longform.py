"""Long recordings end to end and by piece (thunder_speech_amd/longform.py, csrc/longform.hip, csrc/ctc_align_long.hip).
python tools/bench_longform.py [--out profiles/longform.md]

Synthetic audio (0.1 x randn) and random weights, as the other tools.
  * transcription: `transcribe_long` (greedy; chunk 20 s, context 2 s, 16 windows per batch) on one 30-minute and on eight 10-minute recordings, for
    QuartzNet15x5 and the wav2vec2-large geometry, in audio-seconds per second of wall time (host included: plans, tables, decoding), next to the same
    module's `predict` on [16, 20 s] batches at one address in the same run.  The gap is the price of the overlap (20 / 16 of the audio is run) plus
    gather, stitch and the decode of one long row per recording;
  * the gather and stitch launches by device events, next to their HBM floors (bytes read + written / 8 TB/s);
  * ts_ctc_align_long at three shapes, on the first two next to ts_ctc_align on the same tensors in the same run, calls alternating; then the first
    shape again under each explicit states_per_thread (one wave each: what a thread's serial share of a frame costs)."""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

HBM_TBS = 8.0
SR = 16000


def quartznet():
    from thunder_speech_amd.quartznet.compatibility import build_synthetic_quartznet
    return build_synthetic_quartznet(repeat_blocks=3).cuda().eval()


def wav2vec2_large():
    import transformers
    from thunder_speech_amd.blocks import linear_decoder
    from thunder_speech_amd.huggingface.encoder import HuggingFaceEncoderAdapt
    from thunder_speech_amd.huggingface.transform import Wav2Vec2Preprocess
    from thunder_speech_amd.module import BaseCTCModule
    from thunder_speech_amd.text_processing.transform import BatchTextTransformer
    torch.manual_seed(0)
    cfg = transformers.Wav2Vec2Config(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096, feat_extract_norm="layer",
                                      do_stable_layer_norm=True, conv_bias=True, vocab_size=32)
    enc = HuggingFaceEncoderAdapt(transformers.Wav2Vec2Model(cfg), precision="bf16")
    tokens = [chr(97 + i) for i in range(26)] + [" "]
    module = BaseCTCModule(enc, linear_decoder(1024, len(tokens) + 1, 0.0), Wav2Vec2Preprocess(), BatchTextTransformer(tokens=tokens)).cuda().eval()
    module.graph_inference = True
    return module


def wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def transcription(name, module, reps):
    g = torch.Generator().manual_seed(7)
    rows = []
    with torch.no_grad():
        x = (0.1 * torch.randn(16, 20 * SR, generator=g)).cuda()
        for _ in range(3):                                             # eager, captured, replayed
            module.predict(x)
        dt = wall(lambda: module.predict(x), max(reps, 3))
        base = 16 * 20 / dt
        for what, recs in (("1 x 30 min", [30 * 60]), ("8 x 10 min", [10 * 60] * 8)):
            audio = [(0.1 * torch.randn(s * SR + 5, generator=g)).cuda() for s in recs]
            dt = wall(lambda: module.transcribe_long(audio), reps)
            rows.append(f"| {name} | {what} | {sum(recs) / dt:.0f} | {base:.0f} | {sum(recs) / dt / base:.2f} |")
            del audio
    return rows


def events(fn, reps, blocks=5):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / reps * 1e3)
    return best


def plumbing(reps):
    from thunder_speech_amd import longform as LF
    rows = []
    g = torch.Generator().manual_seed(3)
    chunk, spf = 20 * SR, 320
    rec = (0.1 * torch.randn(10 * 60 * SR + 5, generator=g)).cuda()
    audio, begin, _ = LF.pack_recordings([rec])
    for v, f, dtype in ((29, 1001, torch.bfloat16), (32, 999, torch.float32)):
        plan = LF.plan_windows(rec.shape[0], chunk, 100, spf, f)
        windows = torch.tensor([(0, s) for s in plan.starts[:16]], dtype=torch.int64).cuda()
        stage = torch.zeros(16, chunk, device="cuda")
        us = events(lambda: LF.gather_windows(audio, begin, windows, 16, stage), reps)
        floor = 2 * 16 * chunk * 4 / (HBM_TBS * 1e12) * 1e6
        rows.append(f"| ts_longform_gather: 16 windows x 20 s | {us:.1f} | {floor:.1f} | {us / floor:.1f} |")
        win = torch.randn(len(plan), v, f, generator=g).to(dtype).cuda()
        cuts = torch.tensor(LF.cut_table([plan]), dtype=torch.int32).cuda()
        out = torch.zeros(1, v, plan.n_frames, device="cuda")
        lengths = torch.zeros(1, dtype=torch.int32, device="cuda")
        us = events(lambda: LF.stitch_windows(win, cuts, out, lengths), reps)
        floor = plan.n_frames * v * (win.element_size() + 4) / (HBM_TBS * 1e12) * 1e6
        rows.append(f"| ts_longform_stitch: 10 min, {len(plan)} windows, V {v}, {str(dtype).split('.')[-1]} -> f32 [1, {v}, {plan.n_frames}] | {us:.1f} | {floor:.2f} | "
                    f"{us / floor:.0f} |")
    return rows[:1] + rows[1::2]


def aligner(reps):
    from thunder_speech_amd import _lib
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    # the last rows: the first shape again under every explicit block size (one wave each: what a thread's serial share of a frame costs)
    for name, b, t, s, v, both, spt in (("16 x (T 999, S 150, V 32)", 16, 999, 150, 32, True, 0), ("1 x (T 4999, S 700, V 32)", 1, 4999, 700, 32, True, 0),
                                        ("1 x (T 90000, S 25000, V 32)", 1, 90000, 25000, 32, False, 0)) + tuple(
                                            (f"16 x (T 999, S 150, V 32), states_per_thread = {q}", 16, 999, 150, 32, False, q) for q in (16, 32, 64)):
        g = torch.Generator().manual_seed(b * 1000 + t)
        logits = (2 * torch.randn(b, v, t, generator=g)).cuda()
        targets = torch.randint(1, v, (b, s), generator=g, dtype=torch.int32).cuda()
        il = torch.full((b,), t, dtype=torch.int32, device="cuda")
        tl = torch.full((b,), s, dtype=torch.int32, device="cuda")
        path, spans = torch.empty(b, t, dtype=torch.int32, device="cuda"), torch.empty(b, s, 2, dtype=torch.int32, device="cuda")
        logp, score = torch.empty(b, s, device="cuda"), torch.empty(b, device="cuda")
        head = (logits.data_ptr(), b, v, t, t, targets.data_ptr(), s, il.data_ptr(), tl.data_ptr(), 0)
        tail = lambda ws: (path.data_ptr(), spans.data_ptr(), logp.data_ptr(), score.data_ptr(), ws.data_ptr(), st)
        ws_long = torch.empty(L.ts_ctc_align_long_workspace_bytes(b, t, s), dtype=torch.uint8, device="cuda")
        cfg = [C.c_int32(0) for _ in range(3)]
        _lib.check(L.ts_ctc_align_long_launch_config(t, s, spt, v, *[C.addressof(c) for c in cfg]), "ts_ctc_align_long_launch_config")
        calls = {"long": lambda: L.ts_ctc_align_long(*head, spt, *tail(ws_long))}
        if both:
            ws = torch.empty(L.ts_ctc_align_workspace_bytes(b, t, s), dtype=torch.uint8, device="cuda")
            calls["short"] = lambda: L.ts_ctc_align(*head, *tail(ws))
        n = reps if t < 10000 else 2
        best = {k: float("inf") for k in calls}
        for k, f in calls.items():
            _lib.check(f(), k)
        torch.cuda.synchronize()
        for _ in range(3):
            for k, f in calls.items():
                best[k] = min(best[k], events(f, n, blocks=1))
        feasible = int(torch.isfinite(score).sum())
        lo = best["long"]
        old = f"{best['short']:.1f} | {lo / best['short']:.2f}" if both else ("refused (S > 2047) | " if s > 2047 else " | ")
        rows.append(f"| {name} | {cfg[0].value}, {cfg[1].value}, {ws_long.numel() / 2 ** 20:.1f} MiB | {lo:.1f} | {old} | {lo / t * 1e3:.0f} | {feasible} of {b} |")
    return rows


def main():
    ap = argparse.ArgumentParser(description="transcribe_long / gather / stitch / ts_ctc_align_long on one MI355X")
    ap.add_argument("--reps", type=int, default=20, help="calls per timed block of the per-call rows")
    ap.add_argument("--out", default=None, help="also write the tables (markdown) to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_longform: needs an MI355X")
    lines = ["## Transcription", "",
             "`transcribe_long(recordings)` (greedy; chunk 20 s, context 2 s, 16 windows per batch), wall time with the host's share, best of 2 after a "
             "warm-up call; `predict` on one [16, 20 s] batch at a fixed address, best of 3.  Synthetic audio, random weights.", "",
             "| model | recordings | transcribe_long audio-s / s | predict [16, 20 s] audio-s / s | ratio |", "|---|---|---:|---:|---:|"]
    for name, build in (("QuartzNet15x5", quartznet), ("wav2vec2-large geometry (bf16)", wav2vec2_large)):
        module = build()
        lines += transcription(name, module, 2)
        del module
        torch.cuda.empty_cache()
    lines += ["", "## The plumbing launches", "", f"Device events around {a.reps} back-to-back calls, best of 5 blocks; floor = bytes read + written at {HBM_TBS:.0f} TB/s.", "",
              "| call | us | HBM floor us | x floor |", "|---|---:|---:|---:|"] + plumbing(a.reps)
    lines += ["", "## The long aligner", "",
              f"Device events around {a.reps} back-to-back calls (2 at T 90 000), the two aligners alternating, best of 3 blocks after a warm-up call of each; "
              "2 x randn logits, random targets, full lengths.  The last three rows: the first shape under an explicit states_per_thread.", "",
              "| shape | ts_ctc_align_long: states per thread, threads, workspace | ts_ctc_align_long us | ts_ctc_align us | long / short | per frame ns (long) | feasible |",
              "|---|---|---:|---:|---:|---:|---|"] + aligner(a.reps)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
