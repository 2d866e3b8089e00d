"""Long recordings on the CPU: the window plan of thunder_speech_amd/longform.py (every frame from exactly one window, on the recording's grid), its
refusals, the open companion header include_open/thunder_speech_amd/longform.h through `_lib.OPEN` and the built library, and the argument
checks of its launchers (made-up pointers: none of these calls reaches a device call)."""
import ctypes
import os
import re
import subprocess
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 320000                                                          # 20 s at 16 kHz


# ---- the window plan ---------------------------------------------------------------------------------------------------------------------------
def _frames(kind, n, spf):
    """Output frames of a clip of n samples: "conv" = the transformers families' floor((n - 400) / spf) + 1, "mel" = the centred STFT's n // spf + 1."""
    return (n - 400) // spf + 1 if kind == "conv" else n // spf + 1


@pytest.mark.parametrize("kind", ["conv", "mel"])
@pytest.mark.parametrize("spf", [320, 1280])
@pytest.mark.parametrize("n", [CHUNK + 1, "chunk+spf", int(3.1 * CHUNK), 10 * 60 * 16000 + 5])
def test_plan_windows_covers_every_frame_exactly_once_on_the_recordings_grid(n, spf, kind):
    from thunder_speech_amd.longform import plan_windows
    n = CHUNK + spf if n == "chunk+spf" else n
    f, ctx = _frames(kind, CHUNK, spf), 2 * 16000 // spf
    p = plan_windows(n, CHUNK, ctx, spf, f)
    assert p is not None and len(p) >= 2 and p.hop_frames == f - 2 * ctx and p.frames_per_window == f
    assert len(p.starts) == len(p.frames) == len(p.cut_lo) == len(p.cut_hi)
    # all windows start on the grid; the regular ones at w * hop, the last one moved back to end at or after the recording's end
    assert all(s % spf == 0 and s == g * spf for s, g in zip(p.starts, p.frames))
    assert p.frames[:-1] == [w * p.hop_frames for w in range(len(p) - 1)] and p.frames[-2] < p.frames[-1]
    assert n <= p.starts[-1] + CHUNK < n + spf
    # every global frame below T_r is owned by exactly one window and lies inside it
    owner = torch.zeros(p.n_frames, dtype=torch.int32)
    for w in range(len(p)):
        assert p.frames[w] <= p.cut_lo[w] <= p.cut_hi[w] <= p.frames[w] + f
        owner[p.cut_lo[w]: p.cut_hi[w]] += 1
    assert p.cut_lo[0] == 0 and p.cut_hi[-1] == p.n_frames == p.frames[-1] + f and bool((owner == 1).all())
    assert all(p.cut_lo[w + 1] == p.cut_hi[w] == (p.frames[w] + f + p.frames[w + 1]) // 2 for w in range(len(p) - 1))
    # within one frame of the frame count of the recording run whole
    assert 0 <= p.n_frames - _frames(kind, n, spf) <= 1


def test_a_recording_that_fits_one_window_has_no_plan():
    from thunder_speech_amd.longform import plan_windows
    for n in (1, CHUNK - 1, CHUNK):
        assert plan_windows(n, CHUNK, 100, 320, 999) is None
    assert plan_windows(CHUNK + 1, CHUNK, 100, 320, 999) is not None


def test_plan_windows_refusals():
    from thunder_speech_amd.longform import grid_multiple, plan_windows
    with pytest.raises(ValueError, match="hop_frames = 0"):
        plan_windows(10 * CHUNK, CHUNK, 500, 320, 1000)
    with pytest.raises(ValueError, match="hop_frames = -1"):
        plan_windows(CHUNK - 5, CHUNK, 500, 320, 999)                    # refused whatever the recording's length
    # SEW pools squeeze_factor frames, an adapter strides: the hop must be a multiple of the grid's step
    sew = types.SimpleNamespace(squeeze_factor=2, add_adapter=False)
    adapter = types.SimpleNamespace(add_adapter=True, adapter_stride=2, num_adapter_layers=3)
    plain = types.SimpleNamespace(add_adapter=False)
    assert (grid_multiple(sew), grid_multiple(adapter), grid_multiple(plain), grid_multiple(None)) == (2, 8, 1, 1)
    with pytest.raises(ValueError, match="not a multiple of 2"):
        plan_windows(3 * CHUNK, CHUNK, 100, 320, 999, grid_multiple(sew))        # hop 799
    with pytest.raises(ValueError, match="not a multiple of 8"):
        plan_windows(3 * CHUNK, CHUNK, 100, 320, 996, grid_multiple(adapter))    # hop 796
    p = plan_windows(3 * CHUNK + 7, CHUNK, 100, 320, 1000, grid_multiple(adapter))   # hop 800
    assert all(g % 8 == 0 for g in p.frames) and p.starts[-1] + CHUNK >= 3 * CHUNK + 7
    with pytest.raises(ValueError):
        plan_windows(3 * CHUNK, 0, 0, 320, 999)


# ---- the header ----------------------------------------------------------------------------------------------------------------------------------
NAMES = ["ts_longform_abi_version", "ts_longform_gather", "ts_longform_stitch", "ts_ctc_align_long_launch_config", "ts_ctc_align_long_workspace_bytes",
         "ts_ctc_align_long"]
vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64


def test_the_header_is_bound_through_the_open_table():
    from thunder_speech_amd import _lib
    from thunder_speech_amd import build as b
    assert "longform" in _lib.OPEN
    h = _lib.OPEN["longform"]
    assert h.path == os.path.join(ROOT, "include_open", "thunder_speech_amd", "longform.h") and h.path in b.header_deps()
    assert (h.version_define, h.version_function, h.abi_version) == ("TS_LONGFORM_ABI_VERSION", "ts_longform_abi_version", 1)
    code = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(h.path).read(), flags=re.S)
    assert sorted(h.signatures) == sorted(set(re.findall(r"\b(ts_[a-z0-9_]+)\s*\(", code))) == sorted(NAMES)
    assert h.signatures["ts_longform_gather"] == (ctypes.c_int, [vp, vp, i32, vp, i32, vp, i32, i32, vp])
    assert h.signatures["ts_longform_stitch"] == (ctypes.c_int, [vp, i32, i32, i32, i32, vp, vp, i32, i32, vp, vp])
    assert h.signatures["ts_ctc_align_long_launch_config"] == (ctypes.c_int, [i32, i32, i32, i32, vp, vp, vp])
    assert h.signatures["ts_ctc_align_long_workspace_bytes"] == (i64, [i32, i32, i32])
    # ts_ctc_align's arguments with states_per_thread between `blank` and `path`
    align = _lib.COMPANIONS["ctc_align"].signatures["ts_ctc_align"]
    assert h.signatures["ts_ctc_align_long"] == (align[0], align[1][:10] + [i32] + align[1][10:])
    assert (h.defines["TS_CTC_ALIGN_LONG_S_MAX"], h.defines["TS_CTC_ALIGN_LONG_V_MAX"]) == (32767, 2400)
    # nothing of include/ or include_staged/ moved: the header's names are in no other table
    others = [_lib.CORE, *_lib.COMPANIONS.values(), *_lib.STAGED.values(), *_lib.QUEUED.values(), *(o for k, o in _lib.OPEN.items() if k != "longform")]
    assert not [n for o in others for n in o.signatures if n in NAMES]
    text = open(h.path).read()
    for phrase in ("choosing the seams from the data", "streaming input", "transcripts beyond"):
        assert phrase in text                                            # the header names what is out of scope


def test_the_library_exports_every_prototype_and_reports_the_headers_version():
    from thunder_speech_amd import _lib
    from thunder_speech_amd import build as b
    nm = subprocess.run(["nm", "-D", "--defined-only", b.build(verbose=False)], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert not [n for n in NAMES if n not in defined]
    assert _lib.lib().ts_longform_abi_version() == _lib.OPEN["longform"].abi_version == 1


def test_the_two_hip_files_are_picked_up_by_the_build_and_ts_ctc_align_keeps_its_refusal():
    from thunder_speech_amd import _lib
    from thunder_speech_amd import build as b
    assert {"longform.hip", "ctc_align_long.hip"} <= {os.path.basename(p) for p in b.sources()}
    assert _lib.lib().ts_ctc_align_workspace_bytes(1, 10, 2048) == _lib.TS_EUNSUPPORTED


# ---- argument checks -----------------------------------------------------------------------------------------------------------------------------
def _host_cases():
    """(entry point, arguments, expected status) of calls that return before any device call.  Pointers are made-up addresses (never dereferenced
    on these paths): A is 16-byte aligned."""
    A, E, U = 0x10000, -1, -2
    al = lambda lg=A, b=2, v=8, t=50, pitch=64, tg=A, s=10, il=A, tl=A, blank=0, spt=0, path=A, spans=A, logp=A, score=A, ws=A: (
        "ts_ctc_align_long", (lg, b, v, t, pitch, tg, s, il, tl, blank, spt, path, spans, logp, score, ws, None))
    awb = lambda b=2, t=50, s=10: ("ts_ctc_align_long_workspace_bytes", (b, t, s))
    ga = lambda audio=A, rb=A, r=2, win=A, nw=3, out=A, b=4, chunk=100: ("ts_longform_gather", (audio, rb, r, win, nw, out, b, chunk, None))
    st = lambda win=A, bf=0, w=3, v=8, f=50, cuts=A, out=A, r=2, pitch=200, ln=A: ("ts_longform_stitch", (win, bf, w, v, f, cuts, out, r, pitch, ln, None))
    cases = [
        (al(lg=0), E), (al(tg=0), E), (al(il=0), E), (al(tl=0), E), (al(path=0), E), (al(spans=0), E), (al(logp=0), E), (al(score=0), E), (al(ws=0), E),
        (al(b=0), E), (al(v=0), E), (al(t=0), E), (al(s=-1), E), (al(pitch=49), E), (al(blank=-1), E), (al(blank=8), E),
        # states_per_thread: outside {0, 8, 16, 32, 64}; explicit and too small for s_max (2 s_max + 1 > 1024 states_per_thread)
        (al(spt=1), E), (al(spt=4), E), (al(spt=12), E), (al(spt=128), E), (al(spt=-8), E),
        (al(s=4096, spt=8), E), (al(s=8192, spt=16), E), (al(s=16384, spt=32), E), (al(s=32767, spt=32), E),
        # the caps
        (al(s=32768), U), (al(s=40000, spt=64), U), (al(v=2401), U), (al(ws=A + 8), U),
        (awb(b=0), E), (awb(t=0), E), (awb(s=-1), E), (awb(s=32768), U),
        (ga(audio=0), E), (ga(rb=0), E), (ga(win=0), E), (ga(out=0), E), (ga(r=0), E), (ga(nw=-1), E), (ga(b=0), E), (ga(nw=5), E), (ga(chunk=0), E),
        (ga(audio=A + 2), U), (ga(out=A + 2), U), (ga(rb=A + 4), U), (ga(win=A + 4), U),
        (st(win=0), E), (st(cuts=0), E), (st(out=0), E), (st(ln=0), E), (st(w=0), E), (st(v=0), E), (st(f=0), E), (st(r=0), E), (st(pitch=0), E),
        (st(v=65536), E), (st(win=A + 2), U), (st(win=A + 1, bf=1), U), (st(cuts=A + 2), U), (st(out=A + 2), U), (st(ln=A + 2), U),
    ]
    return [(name, args, want) for (name, args), want in cases]


@pytest.mark.parametrize("name,args,want", _host_cases(), ids=lambda v: v if isinstance(v, str) else None)
def test_launchers_refuse_bad_arguments_before_any_device_call(name, args, want):
    from thunder_speech_amd import _lib
    assert (_lib.TS_EINVAL, _lib.TS_EUNSUPPORTED) == (-1, -2)
    assert getattr(_lib.lib(), name)(*args) == want


def _query(L, n_frames, s_max, spt_in, v):
    out = [ctypes.c_int32(-7) for _ in range(3)]
    st = L.ts_ctc_align_long_launch_config(n_frames, s_max, spt_in, v, *[ctypes.addressof(o) for o in out])
    return st, tuple(o.value for o in out)


@pytest.mark.parametrize("states,spt,threads", [(1, 8, 64), (301, 8, 64), (513, 8, 128), (8191, 8, 1024), (8193, 16, 576), (16385, 32, 576),
                                                (32767, 32, 1024), (32769, 64, 576), (50001, 64, 832), (65535, 64, 1024)])
def test_launch_config_chooses_the_smallest_block_under_which_the_states_fit_1024_threads(states, spt, threads):
    from thunder_speech_amd import _lib
    L = _lib.lib()
    s_max = (states - 1) // 2
    lds = lambda th, v: 64 * v + 8 * (th + 1) + 64 + 16
    assert _query(L, 20, s_max, 0, 32) == (0, (spt, threads, lds(threads, 32)))
    assert _query(L, 20, s_max, 64, 1025) == (0, (64, (-(-states // 64) + 63) // 64 * 64, lds((-(-states // 64) + 63) // 64 * 64, 1025)))
    assert _query(L, 20, s_max, 0, 2400)[1][2] <= 160 * 1024               # the class cap fits LDS under the largest workgroup
    # the workspace does not depend on the block: rows of round_up(states, 64) 2-bit codes, and 8 bytes per frame
    assert L.ts_ctc_align_long_workspace_bytes(3, 20, s_max) == 3 * 20 * ((states + 63) // 64 * 16 + 8)


def test_launch_config_refusals_and_64_bit_workspace():
    from thunder_speech_amd import _lib
    L = _lib.lib()
    assert _query(L, 0, 10, 0, 32)[0] == -1 and _query(L, 10, -1, 0, 32)[0] == -1 and _query(L, 10, 10, 0, 0)[0] == -1
    assert _query(L, 10, 10, 7, 32)[0] == -1 and _query(L, 10, 4096, 8, 32)[0] == -1 and _query(L, 10, 4095, 8, 32)[0] == 0
    assert _query(L, 10, 32768, 0, 32)[0] == -2 and _query(L, 10, 10, 0, 2401)[0] == -2 and _query(L, 10, 32767, 0, 2400)[0] == 0
    out = ctypes.c_int32(0)
    assert L.ts_ctc_align_long_launch_config(10, 10, 0, 32, None, ctypes.addressof(out), ctypes.addressof(out)) == -1
    assert L.ts_ctc_align_long_workspace_bytes(1, 90000, 25000) == 90000 * (50048 // 4 + 8) > 2 ** 30


# ---- no CPU path ---------------------------------------------------------------------------------------------------------------------------------
def test_cpu_tensors_are_refused_and_the_keywords_are_checked_before_any_device_work():
    from thunder_speech_amd.ctc_align import forced_align_long
    from thunder_speech_amd.registry import load_pretrained
    module = load_pretrained("QuartzNet5x5_synthetic")
    x = torch.zeros(40000)
    for call in (lambda: module.logits_long(x), lambda: module.transcribe_long([x]), lambda: module.predict_spans_long(x),
                 lambda: module.align_long(x, ["hello"])):
        with pytest.raises(RuntimeError, match="GPU tensors required"):
            call()
    with pytest.raises(RuntimeError, match="GPU tensors required"):
        forced_align_long(torch.zeros(1, 5, 9), torch.tensor([[1, 2]]), torch.tensor([9]), torch.tensor([2]), 0)
    with pytest.raises(ValueError, match="1-D waveform"):
        module.logits_long(torch.zeros(2, 100))
    # the module's own length arithmetic, on the host: a 20 s window of the mel front end at stride 2
    assert module.samples_per_frame == 320 and module._frames_of(CHUNK) == CHUNK // 320 + 1

    class OnGpu(torch.Tensor):                                           # says it lives on a GPU; nothing reaches a kernel before the refusal
        is_cuda = True
    y = torch.zeros(30 * 16000).as_subclass(OnGpu)
    with pytest.raises(ValueError, match="hop_frames"):
        module.logits_long(y, chunk_s=2.0, context_s=1.5)
    with pytest.raises(ValueError, match="give a beam_width"):
        module.transcribe_long(y, hotword_weight=1.0)
