"""CPU-only checks of the boundary: the shared library exports every symbol the header declares, the ctypes
structs match the header, the host-side packers implement the documented fragment layouts, and the module
surface mirrors the reference (state-dict keys, constructor errors).  No kernel is launched here."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "thunder_speech_amd.h")


def _declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ts_[a-z0-9_]+)\s*\(", src)))


def test_library_builds_and_exports_every_declared_symbol():
    from thunder_speech_amd import build as b
    from thunder_speech_amd._lib import EXPORTED_SYMBOLS
    path = b.build(verbose=False)              # hipcc cross-compiles gfx950 without a GPU
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    declared = _declared_functions()
    assert declared and set(declared) == set(EXPORTED_SYMBOLS)
    assert not [s for s in declared if s not in defined]
    # the code object really targets gfx950
    out = subprocess.run(["strings", "-n", "6", path], capture_output=True, text=True).stdout
    assert "gfx950" in out


def test_library_loads_and_answers_version_queries():
    from thunder_speech_amd import _lib
    L = _lib.lib()
    assert L.ts_abi_version() == _lib.ABI_VERSION == 15
    assert L.ts_build_target() == b"gfx950"
    for t in (1, 127, 128, 129, 751, 1501, 2001):
        assert L.ts_time_pitch(t) == _lib.time_pitch(t) and _lib.time_pitch(t) % 128 == 0 and _lib.time_pitch(t) >= t


def test_training_attention_mask_workspace_covers_the_dkv_kernels_reach():
    """The dropout mask is a bitstring of n = batch * heads * t * t bits in the forward's workspace, which the caller may hand to the backward as
    fwd_mask.  The dKV kernels rebuild whole 64-key tiles, keys past t included: the furthest keep8() call belongs to the last row (first bit
    n - t) in the last key tile (k0 = 64 * ((t - 1) // 64)) at sub = 1, half = 1, second run of 8 -- bit e0 = n - t + k0 + 32 + 8 + 16 -- and
    keep8 reads the 32-bit words e0 // 32 and e0 // 32 + 1.  Both paths must size the workspace to hold that word, and so must the part of the
    backward's workspace that holds a re-drawn mask."""
    from thunder_speech_amd import _lib
    L = _lib.lib()
    short = []
    for bh in range(1, 34):
        for t in range(1, 201):
            n = bh * t * t
            e0 = n - t + 64 * ((t - 1) // 64) + 32 + 8 + 16
            need = 4 * (e0 // 32 + 2)                                   # bytes up to and including word e0 // 32 + 1
            for batch, heads in ((bh, 1), (1, bh)):
                c = 64 * heads
                al16 = lambda n: (n + 15) // 16 * 16
                # what precedes the re-drawn mask in the backward's workspace: dO bf16 | D f32 (| the WavLM path's drb records, 95 f32 each)
                front = al16(batch * t * c * 2) + al16(batch * heads * t * 4)
                records = al16(batch * heads * ((t + 63) // 64) * ((t + 31) // 32) * 95 * 4)
                got = (L.ts_w2v_attention_train_fwd_workspace(batch, t, c, heads),
                       L.ts_wavlm_attention_train_fwd_workspace(batch, t, c, heads),
                       L.ts_w2v_attention_train_bwd_workspace(batch, t, c, heads) - front,
                       L.ts_wavlm_attention_train_bwd_workspace(batch, t, c, heads) - front - records)
                if min(got) < need:
                    short.append((batch, heads, t, need, got))
    assert not short, short[:5]


_LAYOUT_PROBE = r'''
#include <stddef.h>
#include <stdio.h>
#include "thunder_speech_amd.h"
#define CLS(x) (__builtin_classify_type(x) == 5 ? "ptr" : \
                _Generic((x), float: "f32", int32_t: "i32", int64_t: "i64", uint64_t: "u64", default: "other"))
int main(void) {
%s
  return 0;
}
'''


def test_ctypes_structs_match_the_c_compilers_layout(tmp_path):
    """sizeof, offsetof and the type class of every field, as the host C compiler lays the header's structs out."""
    from thunder_speech_amd import _lib
    from thunder_speech_amd import build as b
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    structs = (("ts_tcs_desc", _lib.TcsDesc), ("ts_tcs_launch", _lib.TcsLaunch), ("ts_frontend_desc", _lib.FrontendDesc), ("ts_wgrad_item", _lib.WgradItem))
    lines = []
    for struct, cls in structs:
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, flags=re.S).group(1)
        names = [re.findall(r"([a-z_0-9]+)\s*$", part.strip())[0] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
        assert names == [f[0] for f in cls._fields_], struct
        lines.append(f'  {{ static {struct} s; printf("{struct} sizeof %zu\\n", sizeof s);')
        lines += [f'    printf("{struct} {n} %zu %s\\n", offsetof({struct}, {n}), CLS(s.{n}));' for n in names]
        lines.append("  }")
    (tmp_path / "probe.c").write_text(_LAYOUT_PROBE % "\n".join(lines))
    cc = shutil.which("cc") or shutil.which("gcc") or \
        os.path.join(os.path.dirname(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), "..", "lib", "llvm", "bin", "clang")
    exe = str(tmp_path / "probe")
    subprocess.run([cc, "-std=c11", "-I", os.path.join(b.ROOT, "include"), "-o", exe, str(tmp_path / "probe.c")], check=True)
    got = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    cls_of = {ctypes.c_float: "f32", ctypes.c_int32: "i32", ctypes.c_int64: "i64", ctypes.c_uint64: "u64", ctypes.c_void_p: "ptr"}
    want = []
    for struct, cls in structs:
        want.append(f"{struct} sizeof {ctypes.sizeof(cls)}")
        want += [f"{struct} {n} {getattr(cls, n).offset} {cls_of[t]}" for n, t in cls._fields_]
    assert got == want


def test_derived_signatures_pin_every_type_mapping():
    """Read from the header alone (no .so): one entry point per row of the C -> ctypes table."""
    from thunder_speech_amd import _lib
    S, P = _lib.SIGNATURES, ctypes.POINTER
    i32, i64, u64, f32, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float, ctypes.c_void_p
    assert len(S) == 123 and list(S) == _lib.EXPORTED_SYMBOLS
    assert S["ts_abi_version"] == (ctypes.c_int, [])
    assert S["ts_build_target"][0] is ctypes.c_char_p
    assert S["ts_time_pitch"] == (ctypes.c_int, [i32])                                      # int
    assert S["ts_frontend_logmel_ptr"] == (vp, [P(_lib.FrontendDesc), vp])                  # const float* return
    assert S["ts_frontend_workspace_bytes"][0] is i64
    assert S["ts_train_pwconv_wgrad_multi_parts"] == (ctypes.c_int, [i32, i32, i32])         # int32_t return
    assert S["ts_tcs_subblock_fwd"] == (ctypes.c_int, [P(_lib.TcsDesc)] + [vp] * 6)
    assert S["ts_tcs_last_launch"] == (ctypes.c_int, [P(_lib.TcsLaunch)])                    # struct* (an output)
    assert S["ts_train_pwconv_wgrad_multi"][1] == [P(_lib.WgradItem), i32, vp]
    assert S["ts_ctc_launch_config"] == (ctypes.c_int, [i32, i32, vp, vp, vp, vp])           # int32_t* (outputs)
    assert S["ts_frontend_launch_config"] == (ctypes.c_int, [P(_lib.FrontendDesc), vp, vp, vp, vp])
    assert S["ts_gemm_nt_launch_config"] == (ctypes.c_int, [vp, i64, vp, i64, vp, vp, i64, vp, i64, vp, i64, i64, i32, i32, i32, i32] + [vp] * 9)
    assert S["ts_gemm_f32_launch_config"] == (ctypes.c_int, [vp, i64, i64, i64, i64, i64] * 2 + [vp, i64] + [i32] * 7 + [vp] * 7)
    assert [_lib.DEFINES["TS_GEMM_NT_" + n] for n in ("LDS_TWO_ROW", "LDS_TWO_ROW_SILU", "PACKED_HALF_TILE", "PACKED_HALF_TILE_SILU", "EPILOGUE_BF16",
                                                       "EPILOGUE_F32")] == [0, 1, 2, 3, 0, 1]
    args = S["ts_train_dropout"][1]
    assert args[5] is f32 and args[6] is u64 and args[2] is i64
    assert len(S["ts_gemm_f32"][1]) == 23 and S["ts_gemm_f32"][1][:2] == [vp, i64]
    assert S["ts_train_wgrad_reduce_multi"][1] == [vp, vp, vp, vp, i32, vp]                   # void* const*, const int64_t*
    assert S["ts_w2v_mask_embed"][1][1] is vp                                               # const uint8_t*
    assert (_lib.ABI_VERSION, _lib.TS_EINVAL, _lib.TS_EUNSUPPORTED, _lib.GUARD_BYTES) == (15, -1, -2, 1024)
    assert (_lib.TCS_IN_TAILZERO, _lib.TCS_OUT_ZERO_TAIL, _lib.TCS_TAPS_PHASE) == (1, 2, 4)


def test_header_reader_on_snippets():
    from thunder_speech_amd._lib import read_header
    sigs, structs, defines = read_header("""
        #define TS_ANSWER (-42)  /* a constant */
        typedef struct ts_pair { const void *a, *b; int32_t n, m; } ts_pair;
        int64_t ts_split(const ts_pair* p,   /* a comment, (with parentheses) */
                         uint64_t seed, // a line comment
                         void* stream);
    """)
    assert defines == {"TS_ANSWER": -42}
    assert [(n, t) for n, t in structs["ts_pair"]._fields_] == [("a", ctypes.c_void_p), ("b", ctypes.c_void_p), ("n", ctypes.c_int32), ("m", ctypes.c_int32)]
    assert sigs == {"ts_split": (ctypes.c_int64, [ctypes.POINTER(structs["ts_pair"]), ctypes.c_uint64, ctypes.c_void_p])}
    with pytest.raises(ValueError, match=r"ts_sized.*size_t"):
        read_header("int ts_sized(const void* p, size_t n);")
    with pytest.raises(ValueError, match=r"ts_wide.*double"):
        read_header("double ts_wide(void);")


def test_pack_pw_frags_layout():
    from thunder_speech_amd import plan
    w = torch.arange(40 * 70, dtype=torch.float32).reshape(40, 70) / 64.0
    fr = plan.pack_pw_frags(w).float()
    assert fr.shape == (2, 8, 64, 8)          # cout 40 -> 64 (2 tiles), cin 70 -> 128 (8 k-steps)
    for (cot, ks, lane, j) in [(0, 0, 0, 0), (0, 3, 37, 5), (1, 4, 7, 2), (1, 7, 63, 7), (0, 4, 33, 6)]:
        n, h = lane & 31, lane >> 5
        co, ci = cot * 32 + n, ks * 16 + 8 * h + j
        want = float(w[co, ci].to(torch.bfloat16)) if co < 40 and ci < 70 else 0.0
        assert float(fr[cot, ks, lane, j]) == want


@pytest.mark.parametrize("k,stride,dil", [(33, 1, 1), (39, 1, 1), (75, 1, 1), (33, 2, 1), (87, 1, 2), (5, 1, 1), (13, 1, 3)])
def test_pack_dw_taps_is_the_toeplitz_of_the_conv(k, stride, dil):
    """out[t + i] = sum_v row_i[v] * x[t*stride - padl4 + v] must equal the reference depthwise conv."""
    from thunder_speech_amd import plan
    from thunder_speech_amd.blocks import get_same_padding
    pad = get_same_padding(k, stride, dil)
    g = torch.Generator().manual_seed(k)
    w = torch.randn(3, 1, k, generator=g).to(torch.bfloat16).float()
    taps, nk = plan.pack_dw_taps(w, stride, dil, pad)
    assert taps.shape == (64, 4, 4 * nk) and nk % plan.NKP == 0 and nk == plan.dw_ksteps(k, stride, dil, pad)
    x = torch.randn(1, 3, 200, generator=g)
    ref = torch.nn.functional.conv1d(x, w, None, stride, pad, dil, groups=3)[0]
    padl4 = plan.round_up(pad, 4)
    xp = torch.nn.functional.pad(x[0], (padl4, 4 * nk + 8))
    for t in (0, 4, 8, 40):
        for i in range(4):
            if t + i >= ref.shape[1]:
                continue
            win = xp[:, t * stride: t * stride + 4 * nk]
            got = (taps[:3, i].float() * win).sum(-1)
            np.testing.assert_allclose(got.numpy(), ref[:, t + i].numpy(), atol=1e-4)
    assert torch.all(taps[3:] == 0)


def test_tap_fragments_layout():
    from thunder_speech_amd import plan
    taps = torch.arange(128 * 4 * 12, dtype=torch.float32).reshape(128, 4, 12)
    fr = plan.tap_fragments(taps)
    assert fr.shape == (2, 4, 3, 64, 4)
    for (chunk, wave, k, lane) in [(0, 0, 0, 0), (1, 3, 2, 63), (0, 2, 1, 37), (1, 0, 0, 5)]:
        ch, row = chunk * 64 + wave * 16 + lane // 4, lane % 4
        assert torch.equal(fr[chunk, wave, k, lane], taps[ch, row, 4 * k: 4 * k + 4])


def test_state_dict_keys_match_reference_layout():
    """Same keys/shapes as the reference module tree (pinned through the oracle's synthetic state dict, which the
    golden generator loaded strict=True into the real reference QuartznetEncoder)."""
    from oracle import tcs as otcs
    from thunder_speech_amd.quartznet.blocks import QuartznetEncoder
    from thunder_speech_amd.blocks import conv1d_decoder, linear_decoder
    for rb, n in ((1, 225), (3, 635)):
        enc = QuartznetEncoder(repeat_blocks=rb)
        ours = enc.state_dict()
        ref = otcs.synth_encoder_state(otcs.quartznet_arch(repeat_blocks=rb), seed=0)
        assert len(ours) == n and set(ours) == set(ref)
        assert all(tuple(ours[k].shape) == tuple(ref[k].shape) for k in ref)
        enc.load_state_dict(ref, strict=True)
    assert sum(p.numel() for p in QuartznetEncoder(repeat_blocks=3).parameters()) + 1024 * 29 + 29 == 18924381
    assert set(conv1d_decoder(1024, 29).state_dict()) == {"weight", "bias"}
    assert set(linear_decoder(32, 11, 0.1).state_dict()) == {"2.weight", "2.bias"}


def test_frontend_module_surface():
    from thunder_speech_amd.quartznet.transform import FilterbankFeatures, patch_stft
    fb = FilterbankFeatures()
    assert list(fb.state_dict()) == ["1.window", "2.layer.0.fb"]
    assert fb[1].n_fft == 512 and fb[1].hop_length == 160 and fb[1].win_length == 320 and fb[1].stft_func is torch.stft
    assert fb[1].get_sequence_length(torch.tensor([1234.0, 159.0])).tolist() == [8, 1]
    patch_stft(fb)
    with pytest.raises(ValueError):
        FilterbankFeatures(num_cutout_masks=1, num_time_masks=1)
    with pytest.raises(ValueError):
        FilterbankFeatures(n_window_size=0)


def test_error_conventions():
    from thunder_speech_amd.blocks import get_same_padding
    from thunder_speech_amd.finetune import FinetuneCTCModule
    from thunder_speech_amd.quartznet.blocks import InitMode, QuartznetBlock, init_weights
    from thunder_speech_amd.registry import load_pretrained
    with pytest.raises(ValueError):
        get_same_padding(3, 2, 2)
    with pytest.raises(ValueError):
        QuartznetBlock(8, 8, kernel_size=(3,), stride=(2,), dilation=(2,))
    with pytest.raises(ValueError):
        init_weights(torch.nn.Conv1d(2, 2, 1), "bogus")
    init_weights(torch.nn.Conv1d(2, 2, 1), InitMode.kaiming_normal)
    with pytest.raises(KeyError):
        load_pretrained("no_such_checkpoint")
    with pytest.raises(ValueError):
        FinetuneCTCModule("QuartzNet5x5_synthetic", tokens=["a", "b"])
    with pytest.raises(ValueError):
        FinetuneCTCModule("QuartzNet5x5_synthetic", decoder_class=lambda c, n: torch.nn.Conv1d(c, n, 1))
    m = FinetuneCTCModule("QuartzNet5x5_synthetic", decoder_class=lambda c, n: torch.nn.Conv1d(c, n, 1), tokens=["a", "b"])
    assert m.decoder.out_channels == 3 and m.encoder_final_dimension == 1024


def test_compute_paths_refuse_cpu_tensors():
    from thunder_speech_amd.registry import load_pretrained
    m = load_pretrained("QuartzNet5x5_synthetic")
    assert not m.training
    with pytest.raises(RuntimeError, match="no CPU"):
        m.predict(torch.zeros(1, 16000))
    with pytest.raises(RuntimeError, match="no CPU"):
        m.encoder(torch.zeros(1, 64, 50), torch.tensor([50]))


def test_text_transform_known_answers():
    # reference: tests/text/test_transforms.py:41-91
    from thunder_speech_amd.text_processing.transform import BatchTextTransformer
    labels = [" "] + [chr(ord("a") + i) for i in range(26)]
    tt = BatchTextTransformer(labels, blank_token="<blank>", pad_token="<pad>", unknown_token="<unk>",
                              start_token="<bos>", end_token="<eos>")
    ids, lens = tt.encode(["hello world"])
    v = tt.vocab
    assert ids[0].tolist() == [v.stoi["<bos>"], 8, 5, 12, 12, 15, 0, 23, 15, 18, 12, 4, v.stoi["<eos>"]]
    tt2 = BatchTextTransformer(labels + ["'"])
    blank, a, b = tt2.vocab.blank_idx, tt2.vocab.stoi["a"], tt2.vocab.stoi["b"]
    assert tt2.decode_prediction(torch.full((1, 10), blank)) == [""]
    assert tt2.decode_prediction(torch.tensor([[a] * 5 + [b] * 5])) == ["ab"]
    assert tt2.decode_prediction(torch.tensor([[a] * 4 + [blank] + [a] * 4])) == ["aa"]
    assert tt2.num_tokens == 29 and blank == 28


def test_decode_fixture_matches_reference(golden):
    from thunder_speech_amd.text_processing.transform import BatchTextTransformer
    g = golden("decode.npz")
    tt = BatchTextTransformer([str(s) for s in g["labels"]])
    pred = torch.from_numpy(g["pred"])
    assert tt.decode_prediction(pred) == [str(s) for s in g["strings"]]
    assert tt.decode_prediction(pred, remove_repeated=False) == [str(s) for s in g["strings_norep"]]
    ids, lens = tt.encode([str(s) for s in g["texts"]])
    assert np.array_equal(ids.numpy(), g["enc_ids"]) and np.array_equal(lens.numpy(), g["enc_len"])


def _w2v_host_cases():
    """(entry point, arguments, expected status) of calls that return before any launch.  Pointers are made-up addresses (never dereferenced on these
    paths): A is 16-byte aligned, A + 4 / A + 8 are not; 0 is an absent optional argument."""
    A, E, U = 0x10000, -1, -2
    ln = lambda x=A, res=0, xb=0, w=A, b=A, rows=4, c=512, y=A, y16=0: ("ts_w2v_layernorm_fwd", (x, res, xb, w, b, 1e-5, rows, c, 0, y, y16, None))
    lnb = lambda name, x=A, res=0, g=A, dy=A, c=512, dx=A, ws=A: (name, (x, res, g, dy, 1e-5, 4, c, dx, A, A, ws, None))
    glu = lambda x=A, rows=4, c=8, y=A, y16=0: ("ts_w2v_glu_fwd", (x, rows, c, y, y16, None))
    wg = lambda dz=A, x=A, c=128, k=4, groups=2, dw=A, ws=A: ("ts_w2v_posconv_wgrad", (dz, x, 1, 8, c, k, groups, dw, ws, None))
    tr = lambda src=A, res=A, c=128, bias=A, k=4, groups=2, bwd=0, ws=A: ("ts_w2v_posconv_train", (src, res, 1, 8, c, A, bias, k, groups, bwd, A, 0, ws, None))
    pc = lambda name, x=A, c=128, groups=2, prec=0, tail=(A, None): (name, (x, 1, 8, c, A, A, 4, groups, prec, A) + tail)
    rot = lambda x=A, w=A, b=A, t=4, c=128, heads=2, cs=A, prec=1, y=A, yr=A: (
        "ts_conformer_layernorm_rotary_fwd", (x, w, b, 1e-5, 1, t, c, heads, cs, 8, prec, y, yr, None))
    gd = lambda u=A, c=64, k=31, act=2, prec=1: ("ts_conformer_glu_dwconv_fwd", (u, 1, 8, c, A, k, A, A, act, prec, A, None))
    cl = lambda x=A, res=0, y=A, y_op=0, n=64, act=0, prec=0, bias=0, ldc=64: (
        "ts_conformer_linear_fwd", (x, 64, A, 0, bias, res, 64, y, ldc, y_op, 64, 4, n, 64, act, prec, None))
    cases = [
        (("ts_w2v_conv0_workspace_bytes", (0, 16000, 512, 10, 5)), E), (("ts_w2v_conv0_workspace_bytes", (1, 9, 512, 10, 5)), E),
        (("ts_w2v_conv0_fwd", (0, 1, 16000, A, A, A, 512, 10, 5, 1e-5, A, 0, A, None)), E),
        (("ts_w2v_conv0_fwd", (A, 1, 16000, A, A, 0, 512, 10, 5, 1e-5, A, 0, A, None)), E),          # GroupNorm weight without its bias
        (("ts_w2v_conv0_fwd", (A, 1, 16000, A, A, A, 512, 10, 5, 1e-5, 0, 0, A, None)), E),          # no output at all
        (("ts_w2v_conv0_fwd", (A, 1, 16000, A, A, A, 512, 17, 5, 1e-5, A, 0, A, None)), U),          # kernel > 16
        (("ts_w2v_conv_fwd", (A, 1, 2, 512, A, 0, 512, 3, 2, 1, 0, A, 0, 0, None)), E),              # t_in < kernel
        (("ts_w2v_conv_fwd", (A, 1, 50, 512, A, 0, 510, 3, 2, 1, 0, A, 0, 0, None)), U),             # c_out % 4
        (("ts_w2v_conv_fwd", (A, 1, 50, 512, A, 0, 512, 3, 2, 1, 2, A, 0, 0, None)), U),             # precision
        (("ts_w2v_linear_fwd", (A, 63, A, 0, 0, 0, A, 64, 0, 4, 64, 64, 0, 0, 0, None)), E),         # lda < k
        (("ts_w2v_linear_fwd", (A, 64, A, 0, 0, 0, A, 66, 0, 4, 62, 64, 0, 0, 0, None)), U),         # n % 4
        (("ts_w2v_linear_fwd", (A, 64, A, 0, 0, 0, A, 64, 0, 4, 64, 64, 4, 0, 0, None)), U),         # act
        (("ts_w2v_linear_fwd", (A, 64, A, 0, 0, 0, A, 64, 0, 4, 64, 64, 2, 1, 0, None)), E),         # bf16-only result without a bf16 buffer
        (ln(x=0), E), (ln(y=0), E), (ln(rows=0), E), (ln(c=510), U), (ln(c=4100), U),
        (ln(x=A + 4), U), (ln(res=A + 8), U), (ln(xb=A + 4), U), (ln(w=A + 8), U), (ln(b=A + 4), U), (ln(y=A + 8), U), (ln(y16=A + 4), U),
        (ln(y=0, y16=A + 4), U),
        (("ts_w2v_mask_rows", (A, 1, 8, 64, 0, None)), E), (("ts_w2v_mask_rows", (A, 1, 0, 64, A, None)), E),
        (glu(x=0), E), (glu(rows=0), E), (glu(c=6), U), (glu(x=A + 4), U), (glu(y=A + 8), U), (glu(y16=A + 4), U),
        (("ts_w2v_posconv_workspace_bytes", (1, 8, 128, 0)), E),
        (pc("ts_w2v_posconv_fwd", x=0, tail=(0, A, None)), E), (pc("ts_w2v_posconv_fwd", c=130, groups=4, tail=(0, A, None)), E),
        (pc("ts_w2v_posconv_fwd", prec=2, tail=(0, A, None)), U),
        (pc("ts_w2v_groupconv_fwd", x=0), E), (pc("ts_w2v_groupconv_fwd", tail=(0, None)), E), (pc("ts_w2v_groupconv_fwd", prec=-1), U),
        (("ts_w2v_posconv_wgrad_workspace", (1, 8, 0, 4)), E), (("ts_w2v_posconv_train_workspace", (0, 8, 128, 4)), E),
        (wg(dz=0), E), (wg(c=130, groups=4), E), (wg(c=96, groups=2), U), (wg(ws=A + 8), U), (wg(dz=A + 4), U), (wg(x=A + 8), U),
        (tr(src=0), E), (tr(k=1), E), (tr(bias=0), E), (tr(c=96), U), (tr(k=330), U), (tr(ws=A + 8), U), (tr(src=A + 4), U),
        (tr(bias=0, bwd=1, ws=A + 8), U),                                                            # the data gradient takes no bias
        (("ts_w2v_attention_workspace_bytes", (1, 0, 12, 0)), E),
        (("ts_w2v_attention_fwd", (A, 1, 8, 770, 12, 0, 0, A, A, None)), E),                         # c % heads
        (("ts_w2v_attention_fwd", (A, 1, 8, 768, 12, 0, 0, A, 0, None)), E),                         # no workspace
        (("ts_w2v_attention_fwd", (A, 1, 8, 768, 12, 0, 2, A, A, None)), U),
        (lnb("ts_w2v_layernorm_bwd", x=0), E), (lnb("ts_w2v_layernorm_bwd", c=4100), U), (lnb("ts_w2v_layernorm_bwd", x=A + 4), U),
        (lnb("ts_w2v_layernorm_bwd", res=A + 8), U), (lnb("ts_w2v_layernorm_bwd", g=A + 4), U), (lnb("ts_w2v_layernorm_bwd", dy=A + 8), U),
        (lnb("ts_w2v_layernorm_bwd", dx=A + 4), U), (lnb("ts_w2v_layernorm_bwd", ws=A + 8), U),
        (lnb("ts_w2v_layernorm_bwd_set", ws=0), E), (lnb("ts_w2v_layernorm_bwd_set", res=A + 4), U), (lnb("ts_w2v_layernorm_bwd_set", dx=A + 8), U),
        (("ts_w2v_gelu_fwd", (A + 4, 0, 0, A, 8, None)), U), (("ts_w2v_gelu_fwd", (A, A + 8, 4, A, 8, None)), U), (("ts_w2v_gelu_fwd", (A, A, 3, A, 9, None)), U),
        (("ts_w2v_gelu_bwd", (A, 0, 0, A, A + 8, 8, None)), U), (("ts_w2v_gelu_bwd", (A, 0, 0, 0, A, 8, None)), E),
        (("ts_w2v_add", (A, A + 4, A, 8, None)), U), (("ts_w2v_add", (A, A, 0, 8, None)), E),
        (("ts_w2v_ffn_act_cast", (A, 0, 4, 64, 0.0, 1, A + 4, 0, 0, 0, None)), U), (("ts_w2v_ffn_act_cast", (A, A + 8, 4, 64, 0.0, 1, A, 0, 0, 0, None)), U),
        (("ts_w2v_ffn_act_cast", (A, 0, 4, 64, 0.0, 1, 0, A + 2, 32, 32, None)), U), (("ts_w2v_ffn_act_cast", (A, 0, 4, 64, 1.0, 1, A, 0, 0, 0, None)), E),
        (("ts_w2v_ffn_act_bwd", (A, A + 4, 64, A, 0.0, 1, A, 256, None)), U), (("ts_w2v_ffn_act_bwd", (A, 0, 64, A, 0.0, 1, A + 8, 256, None)), U),
        (("ts_w2v_sum_parts", (A + 4, A, 8, 2, None)), E), (("ts_w2v_sum_parts_bias", (A, A + 8, 4, A, 8, 2, None)), E),
        (("ts_w2v_pad_rows", (A, A + 4, 1, 4, 8, 2, 64, 0, None)), U), (("ts_w2v_mask_embed", (A, A, A + 4, 0, 4, 64, None)), U),
        (gd(u=0), E), (gd(u=A + 8), U), (gd(k=30), U), (gd(act=0), U),
        (rot(x=0), E), (rot(t=9), E), (rot(c=130), U), (rot(x=A + 4), U), (rot(w=A + 8), U), (rot(b=A + 4), U), (rot(cs=A + 8), U),
        (rot(y=A + 4), U), (rot(yr=A + 4), U), (rot(prec=0, y=A + 8), U), (rot(prec=0, yr=A + 8), U),
        (cl(x=0), E), (cl(act=3), U), (cl(prec=1, y=0), E), (cl(y_op=A), E), (cl(n=62, ldc=62), U), (cl(y=A + 8), U), (cl(res=A + 4), U),
        (cl(bias=A + 8), U), (cl(res=A, y=A, act=1), U),                                             # activation into the residual stream in place
    ]
    return [(name, args, want) for (name, args), want in cases]


@pytest.mark.parametrize("name,args,want", _w2v_host_cases(), ids=lambda v: v if isinstance(v, str) else None)
def test_w2v_launchers_refuse_bad_arguments_before_any_launch(name, args, want):
    """The argument checks of the wav2vec2 / conformer launchers: TS_EINVAL for missing or inconsistent arguments, TS_EUNSUPPORTED for shapes,
    precisions and pointer alignments no kernel takes (an absent optional pointer is never misaligned)."""
    from thunder_speech_amd import _lib
    assert (_lib.TS_EINVAL, _lib.TS_EUNSUPPORTED) == (-1, -2)
    assert getattr(_lib.lib(), name)(*args) == want



def _tcs_host_cases():
    """(descriptor fields, call arguments, expected status) of ts_tcs_subblock_fwd calls that return before any launch: every field of a valid
    layer plus the change that must be refused.  Pointers are made-up addresses, never dereferenced on these paths."""
    A, E, U = 0x10000, -1, -2
    IN0, OUT0, PHASE = 1, 2, 4                                                                  # TS_TCS_IN_TAILZERO, _OUT_ZERO_TAIL, _TAPS_PHASE
    pw = dict(batch=2, c_in=64, c_out=64, t_in=100, t_out=100, pitch_in=512, pitch_out=512, kernel=1, stride=1, dilation=1, padding=0,
              pw_w=A, bias=A)
    dw = dict(pw, depthwise=1, kernel=5, padding=2, dw_taps=A, dw_ksteps=3)
    res = dict(c_res=64, pitch_res=512, t_res=100, res_stride=1, res_w=A)
    with_res = dict(x_res=A, len_res=A)
    se = dict(pw, flags=IN0 | OUT0, se_y=A, se_gate=A)
    phase = dict(dw, c_out=512, dilation=2, padding=4, flags=IN0 | OUT0 | PHASE)
    cases = [
        # TS_EINVAL: sizes, pitches, conv geometry
        (dict(pw, batch=0), {}, E), (dict(pw, batch=-2), {}, E), (dict(pw, c_in=0), {}, E), (dict(pw, c_in=-64), {}, E),
        (dict(pw, c_out=0), {}, E), (dict(pw, c_out=-1), {}, E), (dict(pw, t_out=0), {}, E), (dict(pw, t_out=-100), {}, E),
        (dict(pw, pitch_out=516), {}, E), (dict(pw, pitch_out=96), {}, E),
        (dict(pw, stride=0), {}, E), (dict(pw, dilation=0), {}, E), (dict(pw, kernel=0), {}, E),
        # ... a residual branch without one of its arguments
        (dict(pw, **res), dict(len_res=A), E), (dict(pw, **res), dict(x_res=A), E), (dict(pw, **dict(res, res_w=0)), with_res, E),
        (dict(pw, **dict(res, pitch_res=516)), with_res, E),
        # ... a depthwise stage without its taps
        (dict(dw, dw_taps=0), {}, E), (dict(dw, dw_ksteps=0), {}, E), (dict(dw, dw_ksteps=-3), {}, E), (dict(dw, dw_ksteps=4), {}, E),
        # TS_EUNSUPPORTED: configurations no kernel takes
        (dict(dw, stride=3), {}, U), (dict(dw, out_fp32=1), {}, U), (dict(pw, out_fp32=1, stride=2), {}, U), (dict(pw, stride=3), {}, U),
        # ... per-tile statistics come out of the masked, stride-1, bf16 pointwise-only launch alone
        (dict(dw, stats=A), {}, U), (dict(pw, stats=A, out_fp32=1), {}, U), (dict(pw, stats=A, stride=2), {}, U),
        (dict(pw, stats=A, **res), with_res, U), (dict(pw, stats=A, flags=IN0), {}, U),
        # ... the squeeze-excite tail lives in the tail-zero, stride-1, bf16 pointwise-only launch without a residual alone
        (dict(se, se_gate=0), {}, U), (dict(dw, flags=IN0 | OUT0, se_y=A, se_gate=A), {}, U), (dict(se, stride=2), {}, U),
        (dict(se, out_fp32=1), {}, U), (dict(se, **res), with_res, U), (dict(se, flags=OUT0), {}, U), (dict(se, flags=IN0), {}, U),
        (dict(se, c_in=80), {}, U), (dict(se, se_y=A + 8), {}, U),
        # ... the phase-split taps belong to dilation-2 layers of more than 256 output channels without a residual
        (dict(phase, dilation=1), {}, U), (dict(phase, **res), with_res, U), (dict(phase, c_out=256), {}, U),
        # ... a depthwise layer whose staged row exceeds 320 elements
        (dict(dw, c_out=256, kernel=229, padding=114, dw_ksteps=60), {}, U),
        # ... among them every stride-2 layer of at most 256 output channels with more than 24 k-steps: the generic kernel's instantiation for
        # 128-frame tiles, stride 2 and taps from global memory is never launched (tests/test_gpu_tcs_kernels.py: UNREACHABLE)
        (dict(dw, c_out=256, kernel=95, stride=2, padding=47, dw_ksteps=27, t_out=50), {}, U),
    ]
    return [pytest.param(fields, args, want, id=f"{i}-{'einval' if want == E else 'eunsupported'}") for i, (fields, args, want) in enumerate(cases)]


@pytest.mark.parametrize("fields,args,want", _tcs_host_cases())
def test_tcs_subblock_refuses_bad_descriptors_before_any_launch(fields, args, want):
    """Every return of ts_tcs_subblock_fwd that precedes a launch (csrc/tcs_dispatch.hip): TS_EINVAL for missing or inconsistent arguments,
    TS_EUNSUPPORTED for valid configurations no kernel takes."""
    from thunder_speech_amd import _lib
    A = 0x10000
    assert (_lib.TS_EINVAL, _lib.TS_EUNSUPPORTED) == (-1, -2)
    d = _lib.TcsDesc(**fields)
    got = _lib.lib().ts_tcs_subblock_fwd(ctypes.byref(d), A, A, args.get("x_res"), args.get("len_res"), A, None)
    assert got == want
    # none of these calls reaches a launcher: the thread's launch record says "nothing launched"
    rec = _lib.TcsLaunch(family=7, grid=7)
    assert _lib.lib().ts_tcs_last_launch(ctypes.byref(rec)) == 0
    assert rec.family == _lib.TCS_LAUNCH_NONE == 0 and bytes(rec) == bytes(_lib.TcsLaunch())


def test_tcs_last_launch_refuses_null_and_starts_as_nothing_launched():
    """ts_tcs_last_launch: TS_EINVAL for a null pointer; on a thread that never called ts_tcs_subblock_fwd the record is TS_TCS_LAUNCH_NONE with
    every field 0 (the record is thread-local), and the families keep their values."""
    import threading
    from thunder_speech_amd import _lib
    L = _lib.lib()
    assert L.ts_tcs_last_launch(None) == _lib.TS_EINVAL
    assert (_lib.TCS_LAUNCH_NONE, _lib.TCS_LAUNCH_GENERIC, _lib.TCS_LAUNCH_SPLIT, _lib.TCS_LAUNCH_LOGITS) == (0, 1, 2, 3)
    assert [n for n, _ in _lib.TcsLaunch._fields_] == ["family", "tt", "nt", "stride", "dw", "out_f32", "tlds", "tz", "xj", "npass", "wm", "dil", "se",
                                                       "grid", "n_tt", "n_z", "n_tiles", "lds_bytes", "xcd"]
    seen = []

    def fresh_thread():
        rec = _lib.TcsLaunch(family=7, xcd=7)
        seen.append((L.ts_tcs_last_launch(ctypes.byref(rec)), bytes(rec)))

    th = threading.Thread(target=fresh_thread)
    th.start()
    th.join()
    assert seen == [(0, bytes(_lib.TcsLaunch()))]


_ASAN_DRIVER = r'''
import ctypes as C, sys
L = C.CDLL(sys.argv[1])
i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
assert L.ts_abi_version() == 15
L.ts_build_target.restype = C.c_char_p
assert L.ts_build_target() == b"gfx950"
assert [L.ts_time_pitch(t) for t in (1, 128, 751, 1501)] == [512, 512, 1152, 1920]
# argument validation returns before any launch: null pointers, non-positive sizes, misaligned pitches (TS_EINVAL = -1, TS_EUNSUPPORTED = -2)
class Desc(C.Structure):
    _fields_ = [(n, i32) for n in ("batch", "c_in", "c_out", "t_in", "t_out", "pitch_in", "pitch_out", "kernel", "stride", "dilation", "padding", "depthwise",
                                   "relu", "out_fp32", "c_res", "pitch_res", "t_res", "res_stride", "dw_ksteps", "flags")] + \
               [(n, vp) for n in ("dw_taps", "dw_taps_raw", "pw_w", "res_w", "pw_w16", "res_w16", "bias", "se_y", "se_gate", "stats")]
d = Desc()
L.ts_tcs_subblock_fwd.argtypes = [C.POINTER(Desc), vp, vp, vp, vp, vp, vp]
assert L.ts_tcs_subblock_fwd(None, None, None, None, None, None, None) == -1
buf = (C.c_char * 4096)()
d.batch, d.c_in, d.c_out, d.t_out, d.pitch_in, d.pitch_out, d.kernel, d.stride, d.dilation = 1, 64, 64, 100, 513, 512, 1, 1, 1
d.pw_w = d.bias = C.addressof(buf)
assert L.ts_tcs_subblock_fwd(C.byref(d), buf, buf, None, None, buf, None) == -1              # pitch_in % 8
d.pitch_in, d.stride, d.dilation = 512, 2, 2
assert L.ts_tcs_subblock_fwd(C.byref(d), buf, buf, None, None, buf, None) == -1              # stride AND dilation
d.stride, d.dilation, d.kernel = 1, 1, 5
assert L.ts_tcs_subblock_fwd(C.byref(d), buf, buf, None, None, buf, None) == -2              # dense K > 1
L.ts_tcs_pointwise_tile_frames.argtypes = [i32, i32, i32]
assert L.ts_tcs_pointwise_tile_frames(32, 512, 501) == 64 and L.ts_tcs_pointwise_tile_frames(0, 512, 501) == -1
L.ts_greedy_decode.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, vp]
assert L.ts_greedy_decode(None, 1, 1, 1, 1, None, None, None, None) == -1
assert L.ts_greedy_decode(buf, 2, 29, 100, 64, buf, buf, buf, None) == -1                     # pitch < frames
L.ts_train_set_deterministic.argtypes = [vp, i64]
assert L.ts_train_set_deterministic(buf, 0) == -1 and L.ts_train_set_deterministic(None, 0) == 0
L.ts_train_pwconv_wgrad_workspace.argtypes = [i32, i32, i32]
L.ts_train_pwconv_wgrad_workspace.restype = i64
assert L.ts_train_pwconv_wgrad_workspace(32, 512, 512) >= 512 * 512
L.ts_train_pwconv_wgrad_multi_parts.argtypes = [i32, i32, i32]
assert 1 <= L.ts_train_pwconv_wgrad_multi_parts(32, 512, 512) <= 32
L.ts_train_dwconv_bwd.argtypes = [vp] * 7 + [i32] * 11 + [vp]
assert L.ts_train_dwconv_bwd(None, None, None, None, None, None, None, 1, 1, 1, 1, 1, 1, 1, 0, 8, 8, 0, None) == -1
L.ts_ctc_workspace_bytes.restype = i64
L.ts_ctc_workspace_bytes.argtypes = [i32, i32, i32, i32]
assert L.ts_ctc_workspace_bytes(32, 501, 160, 29) > 0
print("ASAN-DRIVER-OK")
'''


def test_host_code_is_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """`python -m thunder_speech_amd.build --asan`: the extern "C" launchers compiled host-only with -fsanitize=address,undefined and driven through
    the paths that return before a launch (version queries, argument validation, workspace arithmetic).  Any sanitizer report aborts the child."""
    from thunder_speech_amd import build as b
    path = b.build_asan(verbose=False)
    driver = tmp_path / "asan_driver.py"
    driver.write_text(_ASAN_DRIVER)
    env = dict(os.environ, LD_PRELOAD=b.asan_runtime(), ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    import sys
    r = subprocess.run([sys.executable, str(driver), path], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "ASAN-DRIVER-OK" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
