"""CTC alignment on the CPU (the companion C header: tests/test_abi_headers_host.py): that ctc.hip is left alone, the
argument checks of the two launchers (made-up pointers: none of these calls reaches a launch), the launch-config query at the state thresholds
and on either side of the LDS back-pointer limit, the frame -> seconds properties of BaseCTCModule per model family, `words`, and the refusal of
CPU tensors."""
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ctc_loss_source_is_not_touched_by_the_alignment_kernels():
    """The alignment kernels live in their own file and take nothing from csrc/ctc.hip by inclusion: ts_ctc_loss is compiled from the same text."""
    src = open(os.path.join(ROOT, "thunder_speech_amd", "csrc", "ctc_align.hip")).read()
    assert '#include "thunder_speech_amd/ctc_align.h"' in src and "ctc.hip\"" not in src
    assert "ts_ctc_align" not in open(os.path.join(ROOT, "thunder_speech_amd", "csrc", "ctc.hip")).read()


# ---- argument checks ---------------------------------------------------------------------------------------------------------------------------
def _host_cases():
    """(entry point, arguments, expected status) of calls that return before any launch.  Pointers are made-up addresses (never dereferenced on
    these paths): A is 16-byte aligned."""
    A, E, U = 0x10000, -1, -2
    al = lambda lg=A, b=2, v=8, t=50, pitch=64, tg=A, s=10, il=A, tl=A, blank=0, path=A, spans=A, logp=A, score=A, ws=A: (
        "ts_ctc_align", (lg, b, v, t, pitch, tg, s, il, tl, blank, path, spans, logp, score, ws, None))
    gs = lambda lg=A, b=2, v=8, t=50, pitch=64, il=A, blank=0, tok=A, spans=A, logp=A, counts=A, ws=A: (
        "ts_ctc_greedy_spans", (lg, b, v, t, pitch, il, blank, tok, spans, logp, counts, ws, None))
    awb = lambda b=2, t=50, s=10: ("ts_ctc_align_workspace_bytes", (b, t, s))
    gwb = lambda b=2, t=50: ("ts_ctc_greedy_spans_workspace_bytes", (b, t))
    cases = [
        (al(lg=0), E), (al(tg=0), E), (al(il=0), E), (al(tl=0), E), (al(path=0), E), (al(spans=0), E), (al(logp=0), E), (al(score=0), E), (al(ws=0), E),
        (al(b=0), E), (al(v=0), E), (al(t=0), E), (al(t=-1), E), (al(s=-1), E), (al(pitch=49), E), (al(blank=-1), E), (al(blank=8), E),
        (al(s=2048), U), (al(s=4000), U), (al(ws=A + 8), U),
        (gs(lg=0), E), (gs(tok=0), E), (gs(spans=0), E), (gs(logp=0), E), (gs(counts=0), E), (gs(ws=0), E),
        (gs(b=0), E), (gs(v=0), E), (gs(t=0), E), (gs(pitch=49), E), (gs(blank=-1), E), (gs(blank=8), E), (gs(ws=A + 2), U),
        (awb(b=0), E), (awb(t=0), E), (awb(s=-1), E), (awb(s=2048), U),
        (gwb(b=0), E), (gwb(t=0), E),
    ]
    return [(name, args, want) for (name, args), want in cases]


@pytest.mark.parametrize("name,args,want", _host_cases(), ids=lambda v: v if isinstance(v, str) else None)
def test_launchers_refuse_bad_arguments_before_any_launch(name, args, want):
    from thunder_speech_amd import _lib
    assert (_lib.TS_EINVAL, _lib.TS_EUNSUPPORTED) == (-1, -2)
    assert getattr(_lib.lib(), name)(*args) == want


# ---- the launch-config query -------------------------------------------------------------------------------------------------------------------
def _query(L, n_frames, s_max):
    out = [ctypes.c_int32(-7) for _ in range(4)]
    st = L.ts_ctc_align_launch_config(n_frames, s_max, *[ctypes.addressof(o) for o in out])
    return st, tuple(o.value for o in out)


def _lds(n_frames, s_max, spt, threads, bp):
    states = 2 * s_max + 1
    return 4 * (2 * (states + 4) + states) + 64 + (16 * n_frames * spt * threads // 64 if bp else 0)


@pytest.mark.parametrize("states,spt,threads", [(1, 1, 64), (81, 1, 128), (1023, 1, 1024), (1025, 2, 576), (2047, 2, 1024), (2049, 4, 576), (4095, 4, 1024)])
def test_launch_config_at_the_state_thresholds(states, spt, threads):
    """ts_ctc_loss's thresholds: one state per thread up to 1 024 states, two up to 2 048, four beyond; the same workgroup as ts_ctc_launch_config."""
    from thunder_speech_amd import _lib
    L = _lib.lib()
    s_max = (states - 1) // 2
    st, got = _query(L, 20, s_max)
    assert st == 0 and got == (spt, threads, 1, _lds(20, s_max, spt, threads, True))
    loss = [ctypes.c_int32(-7) for _ in range(4)]
    assert L.ts_ctc_launch_config(20, s_max, *[ctypes.addressof(o) for o in loss]) == 0
    assert (loss[0].value, loss[1].value) == (spt, threads)


@pytest.mark.parametrize("s_max,spt,threads", [(40, 1, 128), (150, 1, 320), (600, 2, 640), (1030, 4, 576)])
def test_launch_config_on_either_side_of_the_lds_limit(s_max, spt, threads):
    """The back-pointers cost 16 bytes per frame and 64-state word; they stay in LDS while rows + back-pointers <= 160 KiB, and the workspace
    holds them (and only then grows by them) from the first frame count beyond."""
    from thunder_speech_amd import _lib
    L = _lib.lib()
    per_frame = 16 * spt * threads // 64
    rows = _lds(0, s_max, spt, threads, False)
    last = (160 * 1024 - rows) // per_frame                            # the longest tensor whose back-pointers fit
    st, got = _query(L, last, s_max)
    assert st == 0 and got == (spt, threads, 1, rows + last * per_frame) and got[3] <= 160 * 1024
    st, got = _query(L, last + 1, s_max)
    assert st == 0 and got == (spt, threads, 0, rows)
    assert L.ts_ctc_align_workspace_bytes(3, last, s_max) == 3 * last * 8
    assert L.ts_ctc_align_workspace_bytes(3, last + 1, s_max) == 3 * (last + 1) * (8 + per_frame)
    if s_max == 150:
        assert last > 999                                              # the wav2vec2 shape of the benchmark keeps its back-pointers in LDS


def test_launch_config_refusals_and_greedy_workspace():
    from thunder_speech_amd import _lib
    L = _lib.lib()
    assert L.ts_ctc_align_abi_version() == 1
    assert _query(L, 0, 10)[0] == -1 and _query(L, 10, -1)[0] == -1 and _query(L, 10, 2048)[0] == -2
    assert _query(L, 10, 2047)[0] == 0
    out = ctypes.c_int32(0)
    assert L.ts_ctc_align_launch_config(10, 10, None, ctypes.addressof(out), ctypes.addressof(out), ctypes.addressof(out)) == -1
    assert L.ts_ctc_greedy_spans_workspace_bytes(3, 751) == 3 * 751 * 8
    assert L.ts_ctc_align_workspace_bytes(70000, 70000, 2047) > 2 ** 32        # 64-bit arithmetic


# ---- frames -> seconds -------------------------------------------------------------------------------------------------------------------------
def test_samples_per_frame_of_the_mel_families():
    from thunder_speech_amd.citrinet.compatibility import build_synthetic_citrinet
    from thunder_speech_amd.registry import load_pretrained
    quartz = load_pretrained("QuartzNet5x5_synthetic")
    assert quartz.samples_per_frame == 320 and quartz.sample_rate == 16000
    citri = build_synthetic_citrinet(filters=[64] * 5, kernel_sizes=[11, 13, 15, 17, 19], strides=[2, 1, 2, 1, 2], n_tokens=16)
    assert citri.samples_per_frame == 1280 and citri.sample_rate == 16000


def test_samples_per_frame_of_the_transformers_families():
    transformers = pytest.importorskip("transformers")
    from thunder_speech_amd.huggingface.compatibility import module_from_huggingface

    class FE:
        return_attention_mask = False
        sampling_rate = 16000

    tiny = dict(hidden_size=64, num_hidden_layers=1, num_attention_heads=4, intermediate_size=128, vocab_size=32, num_conv_pos_embeddings=16,
                num_conv_pos_embedding_groups=4)
    w2v = dict(tiny, conv_dim=(32,) * 7, conv_stride=(5, 2, 2, 2, 2, 2, 2), conv_kernel=(10, 3, 3, 3, 3, 2, 2))
    m = module_from_huggingface(transformers.Wav2Vec2ForCTC(transformers.Wav2Vec2Config(**w2v)), FE())
    assert m.samples_per_frame == 320 and m.sample_rate == 16000
    m = module_from_huggingface(transformers.Wav2Vec2ForCTC(transformers.Wav2Vec2Config(**w2v, add_adapter=True, num_adapter_layers=1,
                                                                                       adapter_stride=2, output_hidden_size=64)), FE())
    assert m.samples_per_frame == 640
    sew = dict(tiny, hidden_size=128, num_attention_heads=2, conv_dim=(32,) * 12 + (64,), conv_stride=(5, 2, 1, 2, 1, 2, 1, 2, 1, 2, 1, 2, 1),
               conv_kernel=(10, 3, 1, 3, 1, 3, 1, 3, 1, 2, 1, 2, 1), squeeze_factor=2)
    m = module_from_huggingface(transformers.SEWForCTC(transformers.SEWConfig(**sew)), FE())
    assert m.samples_per_frame == 320                                   # the squeeze and the upsampler cancel
    FE.sampling_rate = 8000
    m = module_from_huggingface(transformers.Wav2Vec2ForCTC(transformers.Wav2Vec2Config(**w2v)), FE())
    assert m.sample_rate == 8000


# ---- words -------------------------------------------------------------------------------------------------------------------------------------
def _clip(tokens):
    from thunder_speech_amd.ctc_align import AlignedClip, TokenSpan
    return AlignedClip(score=-1.0, tokens=[TokenSpan(t, 0.02 * f0, 0.02 * f1, f0, f1, lp) for t, f0, f1, lp in tokens])


def test_words_merges_character_tokens_at_the_separators():
    from thunder_speech_amd.ctc_align import words
    for sep in (" ", "|", "▁"):
        clip = _clip([("h", 2, 3, -0.5), ("i", 3, 6, -0.25), (sep, 6, 7, -1.0), (sep, 9, 10, -1.0), ("y", 11, 12, -0.125), ("o", 14, 15, -0.5),
                      ("u", 15, 16, -0.25), (sep, 16, 18, -0.5)])
        got = words(clip)
        assert [(w.token, w.start_frame, w.end_frame, w.logp) for w in got] == [("hi", 2, 6, -0.75), ("you", 11, 16, -0.875)]
        assert got[0].start == clip.tokens[0].start and got[0].end == clip.tokens[1].end and got[1].end == clip.tokens[6].end
        assert [t.token for t in clip.tokens][:2] == ["h", "i"]         # the clip's own tokens are left as they were
    assert words(_clip([])) == [] and words(_clip([(" ", 0, 1, -1.0)])) == []


def test_words_starts_a_word_at_a_sentencepiece_prefix():
    from thunder_speech_amd.ctc_align import words
    got = words(_clip([("▁he", 0, 2, -1.0), ("llo", 2, 3, -0.5), ("▁wor", 5, 6, -0.25), ("ld", 8, 9, -0.25), ("▁", 9, 10, -2.0), ("x", 10, 11, -1.0)]))
    assert [(w.token, w.start_frame, w.end_frame, w.logp) for w in got] == [("hello", 0, 3, -1.5), ("world", 5, 9, -0.5), ("x", 10, 11, -1.0)]


# ---- the forward align() / predict_spans() run -------------------------------------------------------------------------------------------------
def test_alignment_forward_runs_in_eval_mode_under_no_grad_and_gives_every_submodule_its_flag_back():
    """A module in train mode whose encoder was put into eval mode (the frozen phase of fine-tuning) keeps both flags; the forward itself sees
    eval mode and no_grad.  The forward is a stub and the waveform a stand-in that only says it lives on a GPU: nothing reaches a kernel."""
    from thunder_speech_amd.registry import load_pretrained
    module = load_pretrained("QuartzNet5x5_synthetic")
    module.train()
    module.encoder.eval()
    seen = []

    def forward(x, lengths):
        seen.append((module.training, module.encoder.training, module.decoder.training, torch.is_grad_enabled(), lengths.tolist()))
        return torch.zeros(2, 29, 5), None

    class OnGpu:
        is_cuda, shape, device = True, (2, 100), torch.device("cpu")

    module.forward = forward
    logits, out_lengths = module._eval_logits(OnGpu(), None)
    assert seen == [(False, False, False, False, [100, 100])]
    assert (module.training, module.encoder.training, module.decoder.training) == (True, False, True)
    assert out_lengths.tolist() == [5, 5]                                # no output lengths: every frame


# ---- no CPU path -------------------------------------------------------------------------------------------------------------------------------
def test_cpu_tensors_are_refused():
    from thunder_speech_amd.ctc_align import forced_align, greedy_spans
    from thunder_speech_amd.registry import load_pretrained
    module = load_pretrained("QuartzNet5x5_synthetic")
    x = torch.zeros(1, 4000)
    with pytest.raises(RuntimeError, match="GPU tensors required"):
        module.align(x, ["hello"])
    with pytest.raises(RuntimeError, match="GPU tensors required"):
        module.predict_spans(x)
    with pytest.raises(RuntimeError, match="GPU tensors required"):
        forced_align(torch.zeros(1, 5, 9), torch.tensor([[1, 2]]), torch.tensor([9]), torch.tensor([2]), 0)
    with pytest.raises(RuntimeError, match="GPU tensors required"):
        greedy_spans(torch.zeros(1, 5, 9))
