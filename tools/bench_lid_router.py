"""The language router (BaseCTCModule.language_router / predict_auto, huggingface/classification.py, csrc/seq_cls.hip) on one MI355X, one process,
precision="bf16", random weights, synthetic audio:
  * an MMS-1B geometry module (hidden 1280, 48 layers, 16 heads, FFN 5120, adapter_attn_dim 16) with a bank of 8 languages, and a classifier at the
    same geometry without adapters (classifier_proj_size 1024, 126 labels): `predict_auto` -- ONE graph: classifier, slots written on the device, ASR
    -- next to the two-step path it replaces: `classifier.predict` (graphed), the labels mapped on the host, `predict_languages` (graphed).  The two
    are timed alternately in blocks by the host clock; every call ends in the device-to-host read of its result;
  * ts_seq_cls_pool at batch x 999 x 1280 next to its HBM floor (h read once) -- rotating over copies of h that together exceed the Infinity Cache
    three times, and on one h that stays in it --, ts_seq_cls_head at 126 and 4017 labels next to its floor (the bf16
    weights read once), by device events.
The tool needs the GPU and does not fall back.
python tools/bench_lid_router.py [--batch 16] [--seconds 20] [--layers 48] [--steps 10] [--slots 8] [--out FILE.md]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tools.bench_mms import HBM_PEAK
from tools.bench_mxfp8 import _blocks

C, A, P, LABELS, VOCAB = 1280, 16, 1024, 126, 154


class _Tok:
    pad_token, unk_token, additional_special_tokens = "<pad>", "<unk>", []

    def __init__(self, n):
        self.tokens = ["<pad>", "<s>", "</s>", "<unk>", "|"] + [chr(0x100 + i) for i in range(n - 5)]

    def get_vocab(self):
        return {t: i for i, t in enumerate(self.tokens)}


def build(a):
    """(ASR module with a full bank and a router, classifier), weights drawn on the device."""
    import transformers
    from thunder_speech_amd.huggingface import classifier_from_huggingface
    from thunder_speech_amd.huggingface.compatibility import module_from_huggingface
    geo = dict(hidden_size=C, num_hidden_layers=a.layers, num_attention_heads=16, intermediate_size=5120, feat_extract_norm="layer", conv_bias=True,
               do_stable_layer_norm=True, pad_token_id=0)
    fe = transformers.Wav2Vec2FeatureExtractor(return_attention_mask=True)
    torch.manual_seed(0)
    with torch.device("cuda"):
        asr = transformers.Wav2Vec2ForCTC(transformers.Wav2Vec2Config(**geo, adapter_attn_dim=A, vocab_size=VOCAB)).eval()
        names = [f"lang{i}" for i in range(LABELS)]
        lid = transformers.Wav2Vec2ForSequenceClassification(transformers.Wav2Vec2Config(
            **geo, classifier_proj_size=P, num_labels=LABELS, id2label=dict(enumerate(names)), label2id={s: i for i, s in enumerate(names)})).eval()
    m = module_from_huggingface(asr, fe, _Tok(VOCAB)).cuda()
    m.language_bank("lang0", capacity=a.slots)
    g = torch.Generator().manual_seed(5)
    for s in range(1, a.slots):
        n = max(16, VOCAB - 9 * s)
        pack = {k: torch.randn(v.shape, generator=g) * (0.02 if "linear_2.weight" in k else v.shape[-1] ** -0.5 if v.dim() == 2 else 0.1)
                for k, v in asr._get_adapters().items() if not k.startswith("lm_head")}
        pack.update({"lm_head.weight": torch.randn(n, C, generator=g) / C ** 0.5, "lm_head.bias": torch.zeros(n)})
        m.language_bank_add(f"lang{s}", pack, _Tok(n).tokens)
    clf = classifier_from_huggingface(lid, fe).cuda()
    m.language_router(clf)                                              # the identity: labels lang0 .. lang7 are the bank's languages
    m.graph_inference = True
    return m, clf


def time_router(a):
    m, clf = build(a)
    x = (0.1 * torch.randn(a.batch, 16000 * a.seconds, generator=torch.Generator().manual_seed(0))).cuda()
    bank_names = set(m.language_bank_names())

    def auto():
        return m.predict_auto(x)

    def two_step():
        langs = [s if s in bank_names else None for s in clf.predict(x)]
        return m.predict_languages(x, langs), langs
    res = {"predict_auto (one graph)": [], "classifier.predict + host mapping + predict_languages (two graphs)": []}
    with torch.no_grad():
        for f in (auto, two_step):
            for _ in range(5):                                          # captures (predict()'s graph arrives at the second sighting), then replays
                out = f()
        routed = auto()[1]
        for _ in range(a.blocks):
            for label, f in zip(res, (auto, two_step)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    f()
                torch.cuda.synchronize()
                res[label].append((time.perf_counter() - t0) / a.steps * 1e3)
    return res, routed


def time_launches(a, t=999, reps=50):
    from thunder_speech_amd import _lib
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    b = a.batch
    g = torch.Generator().manual_seed(4)
    h = torch.randn(b, t, C, generator=g).cuda()
    # the pool twice: on ONE h (82 MB at 16 clips: it stays in the 256 MB Infinity Cache between launches) and rotating over enough copies that
    # every launch reads an h last touched more than a cache's worth of bytes ago, which is what the encoder in front of it leaves
    n_rot = -(-3 * 256 * 2 ** 20 // (b * t * C * 4)) + 1
    hs = [h] + [h.clone() for _ in range(n_rot - 1)]
    turn = [0]

    def pool_rotating():
        turn[0] = (turn[0] + 1) % n_rot
        return L.ts_seq_cls_pool(hs[turn[0]].data_ptr(), b, t, C, None, None, 0, partials.data_ptr(), s)
    partials = torch.empty(L.ts_seq_cls_pool_workspace_bytes(b, t, C), dtype=torch.uint8, device="cuda")
    ws = torch.empty(L.ts_seq_cls_head_workspace_bytes(b, P), dtype=torch.uint8, device="cuda")
    pw, pb = (torch.randn(P, C, generator=g) / C ** 0.5).to(torch.bfloat16).cuda(), torch.zeros(P).cuda()
    top1, logp, slot = torch.empty(b, dtype=torch.int32, device="cuda"), torch.empty(b, device="cuda"), torch.empty(b, dtype=torch.int32, device="cuda")
    calls = {f"ts_seq_cls_pool, rotating over {n_rot} h ({n_rot * b * t * C * 4 / 2 ** 20:.0f} MiB): from HBM": pool_rotating,
             "ts_seq_cls_pool, one h: from the Infinity Cache": lambda: L.ts_seq_cls_pool(h.data_ptr(), b, t, C, None, None, 0, partials.data_ptr(), s)}
    floors = {k: b * t * C * 4 for k in calls}
    keep = []
    for n in (126, 4017):
        cw, cb = (torch.randn(n, P, generator=g) / P ** 0.5).to(torch.bfloat16).cuda(), torch.zeros(n).cuda()
        cs, logits = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.empty(b, n, device="cuda")
        keep.append((cw, cb, cs, logits))
        name = f"ts_seq_cls_head, {n} labels"
        calls[name] = lambda cw=cw, cb=cb, cs=cs, logits=logits, n=n: L.ts_seq_cls_head(
            partials.data_ptr(), b, t, C, pw.data_ptr(), pb.data_ptr(), P, cw.data_ptr(), cb.data_ptr(), n, cs.data_ptr(), ws.data_ptr(),
            logits.data_ptr(), top1.data_ptr(), logp.data_ptr(), slot.data_ptr(), 1, s)
        floors[name] = (P * C + n * P) * 2
    return _blocks(calls, reps), floors


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seconds", type=int, default=20)
    ap.add_argument("--layers", type=int, default=48)
    ap.add_argument("--steps", type=int, default=10, help="timed calls per block")
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--out", default=None, help="also write the tables (markdown) to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lid_router: needs an MI355X")
    box = torch.cuda.get_device_name(0)
    res, routed = time_router(a)
    lines = [f"one process on one {box}; precision=\"bf16\", {a.batch} x {a.seconds} s, {a.layers} layers, 1280 hidden / 16 heads / 5120 FFN, random weights; "
             f"ASR: adapter 16, {VOCAB} classes, a bank of {a.slots} languages; classifier: no adapters, projector {P}, {LABELS} labels; a call = everything "
             f"up to the strings on the host; 5 warm-up calls each, then {a.blocks} blocks of {a.steps} calls by the host clock, the two paths alternated", "",
             "| path | ms per call (blocks) | best ms |", "|---|---|---:|"]
    for label, ms in res.items():
        lines.append(f"| {label} | {' / '.join(f'{v:.2f}' for v in ms)} | {min(ms):.2f} |")
    best = [min(v) for v in res.values()]
    lines += ["", f"predict_auto against the two-step path: {best[0] - best[1]:+.2f} ms per call ({best[0] / best[1]:.4f} x); languages routed: "
              f"{sorted(set(routed))} (random weights)"]
    times, floors = time_launches(a)
    lines += ["", f"per launch: {a.batch} clips x 999 frames x 1280 (device events, 3 blocks of 50 launches, the calls alternated); HBM floor at "
              f"{HBM_PEAK / 1e12:.0f} TB/s: pool = h read once in f32; head = the bf16 projector ({P} x 1280) and classifier read once:", "",
              "| launch | us per call (blocks) | best us | floor MB | HBM floor us | best / floor |", "|---|---|---:|---:|---:|---:|"]
    for k, us in times.items():
        fl = floors[k] / HBM_PEAK * 1e6
        lines.append(f"| {k} | {' / '.join(f'{v:.1f}' for v in us)} | {min(us):.1f} | {floors[k] / 1e6:.2f} | {fl:.2f} | {min(us) / fl:.1f} |")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
