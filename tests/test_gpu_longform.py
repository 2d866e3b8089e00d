"""BaseCTCModule.logits_long / transcribe_long / predict_spans_long / align_long through two model families (a tiny QuartzNet on the mel front end
and a tiny wav2vec2 with a layer-norm feature extractor and an attention mask), random weights, chunk_s=2.0, context_s=0.25, batch_size=4 and
recordings of 1.5 s (fits one window), 5.3 s and 9.1 s.

The restatement of logits_long cuts the same windows with numpy, runs the same batches through `module(x, lengths)` and stitches on the host by the
plan: stitching copies, so equality is bit for bit."""
import json

import numpy as np
import pytest
import torch

CHUNK_S, CONTEXT_S, BATCH = 2.0, 0.25, 4
SECONDS = (1.5, 5.3, 9.1)


def _quartznet():
    from oracle import tcs as otcs
    from thunder_speech_amd.quartznet.compatibility import build_synthetic_quartznet
    arch = otcs.quartznet_arch(repeat_blocks=1)
    module = build_synthetic_quartznet(repeat_blocks=1, encoder_state=otcs.synth_encoder_state(arch, seed=0, calibrate=True),
                                       decoder_state=otcs.synth_decoder_state(1024, 29, seed=1, gain=4.0))
    return module.cuda().eval()


def _wav2vec2(tmp_path):
    transformers = pytest.importorskip("transformers")
    from thunder_speech_amd.huggingface.compatibility import module_from_huggingface
    tokens = ["<pad>", "<s>", "</s>", "<unk>", "|"] + [chr(97 + i) for i in range(26)] + ["'"]
    vocab = tmp_path / "vocab.json"
    vocab.write_text(json.dumps({t: i for i, t in enumerate(tokens)}))
    tokenizer = transformers.Wav2Vec2CTCTokenizer(str(vocab))
    torch.manual_seed(3)
    cfg = transformers.Wav2Vec2Config(vocab_size=len(tokens), hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128,
                                      conv_dim=(32, 32, 32), conv_stride=(5, 2, 2), conv_kernel=(10, 3, 2), num_conv_pos_embeddings=16,
                                      num_conv_pos_embedding_groups=4, pad_token_id=0, mask_time_prob=0.0, feat_extract_norm="layer",
                                      do_stable_layer_norm=True, conv_bias=True)
    model = transformers.Wav2Vec2ForCTC(cfg).eval()
    with torch.no_grad():
        model.lm_head.weight.mul_(20.0)                                # a head that prefers something: the greedy transcript is not empty
    module = module_from_huggingface(model, transformers.Wav2Vec2FeatureExtractor(return_attention_mask=True), tokenizer).cuda().eval()
    module.graph_inference = True                                      # the mel families capture on their own; this one is asked to
    return module


@pytest.fixture(scope="module", params=["quartznet", "wav2vec2"])
def setup(request, tmp_path_factory):
    """The module, its recordings, and ONE logits_long of them, shared by the tests below and left unchanged."""
    module = _quartznet() if request.param == "quartznet" else _wav2vec2(tmp_path_factory.mktemp("w2v"))
    rng = np.random.Generator(np.random.PCG64(11))
    sr = module.sample_rate
    recs = [torch.from_numpy((0.1 * rng.standard_normal(int(s * sr) + k)).astype(np.float32)).cuda() for k, s in enumerate(SECONDS)]
    other = torch.from_numpy((0.1 * rng.standard_normal((2, 12000))).astype(np.float32)).cuda()
    with torch.no_grad():
        before = [module.predict(other) for _ in range(3)]              # eager, captured, replayed: predict's graph for another shape
    graphs_before = module.__dict__["_infer_graphs"]
    n_before = graphs_before[1].count() + graphs_before[2].count()
    ll = module.logits_long(recs, chunk_s=CHUNK_S, context_s=CONTEXT_S, batch_size=BATCH)
    return dict(family=request.param, module=module, recs=recs, ll=ll, other=other, before=before, n_before=n_before)


def _host_restatement(module, recs, plans):
    """The window batches cut with numpy, run through module(x, lengths), stitched by the plan on the host."""
    chunk = plans[1].chunk_samples
    wins = []
    for r, p in zip(recs, plans):
        if p is None:
            continue
        x = r.cpu().numpy()
        for s in p.starts:
            w = np.zeros(chunk, np.float32)
            piece = x[s: s + chunk]
            w[: len(piece)] = piece
            wins.append(w)
    n_win = len(wins)
    wins += [np.zeros(chunk, np.float32)] * (-n_win % BATCH)
    outs = []
    full = torch.full((BATCH,), chunk, dtype=torch.int32, device="cuda")
    with torch.no_grad():
        for k in range(0, len(wins), BATCH):
            outs.append(module(torch.from_numpy(np.stack(wins[k: k + BATCH])).cuda(), full)[0].float().cpu())
    win_logits = torch.cat(outs)[:n_win]
    t_max = max(p.n_frames for p in plans if p is not None)
    rows, lengths, w = [], [], 0
    for r, p in zip(recs, plans):
        if p is None:
            with torch.no_grad():
                lg, ln = module(r[None], torch.full((1,), r.shape[0], dtype=torch.int32, device="cuda"))
            row = torch.zeros(lg.shape[1], t_max)
            row[:, : lg.shape[-1]] = lg[0].float().cpu()
            rows.append(row)
            lengths.append(int(ln[0]) if ln is not None else lg.shape[-1])
            continue
        row = torch.zeros(win_logits.shape[1], t_max)
        for i in range(len(p)):
            row[:, p.cut_lo[i]: p.cut_hi[i]] = win_logits[w + i][:, p.cut_lo[i] - p.frames[i]: p.cut_hi[i] - p.frames[i]]
        w += len(p)
        rows.append(row)
        lengths.append(p.n_frames)
    return torch.stack(rows), lengths


@pytest.mark.gpu
def test_logits_long_equals_the_host_restatement_bit_for_bit(setup):
    module, recs, ll = setup["module"], setup["recs"], setup["ll"]
    spf, sr = module.samples_per_frame, module.sample_rate
    assert ll.plans[0] is None and [len(p) for p in ll.plans[1:]] == [4, 6]
    assert all(p.chunk_samples == int(CHUNK_S * sr) and p.hop_frames == p.frames_per_window - 2 * int(CONTEXT_S * sr / spf) for p in ll.plans[1:])
    want, lengths = _host_restatement(module, recs, ll.plans)
    assert ll.logits.dtype == torch.float32 and ll.lengths.dtype == torch.int32 and ll.lengths.cpu().tolist() == lengths
    assert torch.equal(ll.logits.cpu().view(torch.int32), want.view(torch.int32))
    # the recording's grid: within one frame of the recording run whole
    for r, n in zip(recs[1:], lengths[1:]):
        assert 0 <= n - module._frames_of(r.shape[0]) <= 1
    # the short recording's row is module(x[None]) itself
    with torch.no_grad():
        lg, _ = module(recs[0][None], torch.full((1,), recs[0].shape[0], dtype=torch.int32, device="cuda"))
    assert lengths[0] == lg.shape[-1] and torch.equal(ll.logits[0, :, : lengths[0]], lg[0].float()) and not bool(ll.logits[0, :, lengths[0]:].any())


@pytest.mark.gpu
def test_transcribe_long_is_the_existing_decoders_on_the_stitched_logits(setup):
    from thunder_speech_amd import ctc_align as A
    from thunder_speech_amd import ctc_beam as B
    module, recs, ll = setup["module"], setup["recs"], setup["ll"]
    blank = module.text_transform.vocab.blank_idx
    kw = dict(chunk_s=CHUNK_S, context_s=CONTEXT_S, batch_size=BATCH)
    got = module.transcribe_long(recs, **kw)
    gs = A.greedy_spans(ll.logits, ll.lengths, blank)
    assert got == module.text_transform.decode_collapsed(gs.tokens, gs.counts) and len(got) == 3
    with torch.no_grad():
        assert got[0] == module.predict(recs[0][None])[0] == module.transcribe_long(recs[0], **kw)[0]
    assert setup["family"] != "wav2vec2" or all(len(s) > 0 for s in got)
    beam = module.transcribe_long(recs, beam_width=4, **kw)
    res = B.beam_search(ll.logits, ll.lengths, blank, 4, 8, 1)
    ids, counts = A._to_host(res.tokens[:, 0], res.lengths[:, 0])
    assert beam == module.text_transform.decode_collapsed(torch.from_numpy(ids), torch.from_numpy(counts))
    # predict_spans_long: the same greedy tokens, with times on the recording's grid
    spf, sr = module.samples_per_frame, module.sample_rate
    clips = module.predict_spans_long(recs, **kw)
    for b, clip in enumerate(clips):
        text = "".join(t.token for t in clip.tokens).replace("▁", " ").replace("|", " ")
        assert module.text_transform.vocab.remove_special_tokens(text) == got[b]
        assert all(t.start == t.start_frame * spf / sr and t.end == t.end_frame * spf / sr and t.end_frame <= int(ll.lengths[b]) for t in clip.tokens)
    assert setup["family"] != "wav2vec2" or max(t.end for t in clips[2].tokens) > CHUNK_S      # beyond the first window: absolute times


@pytest.mark.gpu
def test_align_long_gives_absolute_times_and_minus_inf_for_a_text_that_cannot_fit(setup):
    from thunder_speech_amd import ctc_align as A
    module, recs, ll = setup["module"], setup["recs"], setup["ll"]
    spf, sr = module.samples_per_frame, module.sample_rate
    kw = dict(chunk_s=CHUNK_S, context_s=CONTEXT_S, batch_size=BATCH)
    texts = ["abc", "hello world", "a" * (int(ll.lengths[2]) + 1)]
    clips = module.align_long(recs, texts, **kw)
    y, y_len = module.text_transform.encode(texts, device="cuda")
    al = A.forced_align_long(ll.logits, y, ll.lengths, y_len, module.text_transform.vocab.blank_idx)
    short = max(int(y_len[0]), int(y_len[1]))                          # forced_align's twin, on the transcripts that one takes
    old = A.forced_align(ll.logits[:2], y[:2, :short].contiguous(), ll.lengths[:2], y_len[:2], module.text_transform.vocab.blank_idx)
    assert torch.equal(al.path[:2], old.path) and torch.equal(al.spans[:2, :short], old.spans)
    spans, score = al.spans.cpu().numpy(), al.score.cpu().numpy()
    itos = module.text_transform.vocab.itos
    for b in range(2):
        assert np.isfinite(score[b]) and abs(clips[b].score - float(score[b])) <= 1e-5 * abs(float(score[b]))
        assert len(clips[b].tokens) == int(y_len[b])
        for j, tok in enumerate(clips[b].tokens):
            assert (tok.token, tok.start_frame, tok.end_frame) == (itos[int(y[b, j])], int(spans[b, j, 0]), int(spans[b, j, 1]))
            assert tok.start == tok.start_frame * spf / sr and tok.end == tok.end_frame * spf / sr
            assert 0 <= tok.start_frame < tok.end_frame <= int(ll.lengths[b])
    assert clips[2].score == float("-inf") and clips[2].tokens == []


@pytest.mark.gpu
def test_a_second_call_replays_the_captured_graph_and_predicts_graphs_stay(setup):
    module, recs, ll = setup["module"], setup["recs"], setup["ll"]
    graphs = module.__dict__.get("_infer_graphs")
    assert graphs is not None
    chunk = ll.plans[1].chunk_samples

    def window_graphs():                                               # the captured graphs whose waveform argument is [BATCH, chunk]
        return {k: e for g in graphs[1:3] for k, e in g._graphs.items() if k[0][0] == (BATCH, chunk)}

    captured = window_graphs()
    assert len(captured) >= 1                                           # the window batches went through a captured graph of their one signature
    assert graphs[1].count() + graphs[2].count() >= setup["n_before"] + 1
    stage = module.__dict__["_long_stages"]
    again = module.logits_long(recs, chunk_s=CHUNK_S, context_s=CONTEXT_S, batch_size=BATCH)
    after = window_graphs()
    assert module.__dict__.get("_infer_graphs") is graphs and after.keys() == captured.keys() and all(after[k] is captured[k] for k in after)
    assert module.__dict__["_long_stages"] is stage and len(stage) == 1 and any(k[-1][0] == next(iter(stage.values())).data_ptr() for k in after)
    assert torch.equal(again.logits.view(torch.int32), ll.logits.view(torch.int32)) and torch.equal(again.lengths, ll.lengths)
    count = graphs[1].count() + graphs[2].count()
    # predict's graph for another shape is still there and gives what it gave
    with torch.no_grad():
        assert module.predict(setup["other"]) == setup["before"][0] == setup["before"][2]
    assert graphs[1].count() + graphs[2].count() == count


@pytest.mark.gpu
def test_a_text_beyond_2047_tokens_aligns_to_a_minute_of_audio(setup):
    """ts_ctc_align refuses this transcript; align_long takes it through ts_ctc_align_long on the stitched logits of 13 windows."""
    from thunder_speech_amd import ctc_align as A
    module = setup["module"]
    spf, sr = module.samples_per_frame, module.sample_rate
    rng = np.random.Generator(np.random.PCG64(5))
    rec = torch.from_numpy((0.1 * rng.standard_normal(60 * sr)).astype(np.float32)).cuda()
    letters = "abcdefghijklmnopqrstuvwxyz"
    text = "".join(letters[(7 * i + i // 26) % 26] for i in range(2100))                      # no equal neighbours: 2 100 frames suffice
    clip, = module.align_long(rec, [text], chunk_s=5.0, context_s=0.5, batch_size=BATCH)
    assert np.isfinite(clip.score) and [t.token for t in clip.tokens] == list(text)
    frames = [(t.start_frame, t.end_frame) for t in clip.tokens]
    assert all(a < b for a, b in frames) and all(frames[j][1] <= frames[j + 1][0] for j in range(len(frames) - 1))
    assert frames[-1][1] <= 60 * sr // spf + 2 and clip.tokens[-1].end > 30.0 and clip.tokens[-1].end == frames[-1][1] * spf / sr
    y, y_len = module.text_transform.encode([text], device="cuda")
    with pytest.raises(NotImplementedError):
        A.forced_align(torch.zeros(1, 32, 3000, device="cuda"), y, torch.tensor([3000]), y_len, 0)
