"""The C ABI's headers on the CPU, from one table: the core header include/thunder_speech_amd.h and the companions in include/thunder_speech_amd/.
Per companion the table pins its exact names, its version and the exact ctypes signatures; from it every companion is checked against
`_lib.read_header`, `_lib.COMPANIONS`, the loaded library and the built library's symbols, and all fifteen headers against each other (no name
twice), against the directory (exactly these files) and against build.needs_build() (a newer header makes the library stale)."""
import ctypes
import glob
import itertools
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
CORE = os.path.join(INCLUDE, "thunder_speech_amd.h")

vp, i32, i64, u64, f32, cint = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float, ctypes.c_int

# stem -> names: every ts_* name the header declares;  version: its TS_*_ABI_VERSION;  signatures: exact (restype, argtypes);  argtypes / restypes:
# where only that half is pinned;  out_of_scope: phrases the header's text must carry (it names what it leaves out)
COMPANIONS = {
    "conformer": dict(
        names=["ts_conformer_abi_version", "ts_conformer_glu_dwconv_fwd", "ts_conformer_layernorm_rotary_fwd", "ts_conformer_linear_fwd"],
        version=1,
        argtypes={
            "ts_conformer_glu_dwconv_fwd": [vp, i32, i32, i32, vp, i32, vp, vp, i32, i32, vp, vp],
            "ts_conformer_layernorm_rotary_fwd": [vp, vp, vp, f32, i32, i32, i32, i32, vp, i32, i32, vp, vp, vp],
            "ts_conformer_linear_fwd": [vp, i64, vp, vp, vp, vp, i64, vp, i64, vp, i64, i64, i32, i32, i32, i32, vp],
        }),
    "conformer_train": dict(
        names=["ts_conformer_train_abi_version", "ts_conformer_glu_dwconv_train_fwd_workspace", "ts_conformer_glu_dwconv_train_fwd",
               "ts_conformer_bn_stats", "ts_conformer_bn_act_cast", "ts_conformer_bn_act_bwd_sums_workspace", "ts_conformer_bn_act_bwd_sums",
               "ts_conformer_glu_dwconv_train_bwd_workspace", "ts_conformer_glu_dwconv_train_bwd", "ts_conformer_rotary_bwd",
               "ts_conformer_ffn_act_cast", "ts_conformer_ffn_act_bwd"],
        version=1,
        signatures={
            "ts_conformer_train_abi_version": (cint, []),
            "ts_conformer_glu_dwconv_train_fwd_workspace": (i64, [i32, i32, i32]),
            "ts_conformer_glu_dwconv_train_fwd": (cint, [vp, i32, i32, i32, vp, i32, vp, vp, vp]),
            "ts_conformer_bn_stats": (cint, [vp, i32, i32, i32, f32, vp, vp, vp]),
            "ts_conformer_bn_act_cast": (cint, [vp, vp, vp, vp, i64, i32, i32, vp, vp, i64, i64, vp]),
            "ts_conformer_bn_act_bwd_sums_workspace": (i64, [i64, i32]),
            "ts_conformer_bn_act_bwd_sums": (cint, [vp, vp, vp, vp, vp, i64, i32, i32, vp, vp, vp, vp]),
            "ts_conformer_glu_dwconv_train_bwd_workspace": (i64, [i32, i32, i32, i32]),
            "ts_conformer_glu_dwconv_train_bwd": (cint, [vp, vp, vp, i32, i32, i32, vp, i32, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp]),
            "ts_conformer_rotary_bwd": (cint, [vp, vp, i32, i32, i32, vp, i32, vp, vp]),
            "ts_conformer_ffn_act_cast": (cint, [vp, vp, i64, i32, i32, f32, u64, vp, vp, i64, i64, vp]),
            "ts_conformer_ffn_act_bwd": (cint, [vp, vp, i32, i32, vp, f32, u64, vp, i64, vp]),
        }),
    "ctc_align": dict(
        names=["ts_ctc_align_abi_version", "ts_ctc_align_launch_config", "ts_ctc_align_workspace_bytes", "ts_ctc_align", "ts_ctc_greedy_spans",
               "ts_ctc_greedy_spans_workspace_bytes"],
        version=1,
        signatures={
            "ts_ctc_align_abi_version": (cint, []),
            "ts_ctc_align_launch_config": (cint, [i32, i32, vp, vp, vp, vp]),
            "ts_ctc_align_workspace_bytes": (i64, [i32, i32, i32]),
            "ts_ctc_align": (cint, [vp, i32, i32, i32, i32, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp]),
            "ts_ctc_greedy_spans_workspace_bytes": (i64, [i32, i32]),
            "ts_ctc_greedy_spans": (cint, [vp, i32, i32, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp]),
        }),
    "ctc_beam": dict(
        names=["ts_ctc_beam_abi_version", "ts_ctc_beam_launch_config", "ts_ctc_beam_workspace_bytes", "ts_ctc_beam_search"],
        version=1,
        signatures={
            "ts_ctc_beam_abi_version": (cint, []),
            "ts_ctc_beam_launch_config": (cint, [i32, i32, i32, vp, vp, vp]),
            "ts_ctc_beam_workspace_bytes": (i64, [i32, i32, i32, i32]),
            "ts_ctc_beam_search": (cint, [vp, i32, i32, i32, i32, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp]),
        },
        out_of_scope=("language-model fusion", "lexicon constraints", "word-insertion bonuses", "beams wider than 64", "word-level timestamps")),
    "ctc_beam_lm": dict(
        names=["ts_ctc_beam_lm_abi_version", "ts_ctc_beam_lm_launch_config", "ts_ctc_beam_lm_workspace_bytes", "ts_ctc_beam_lm_search"],
        version=1,
        signatures={
            "ts_ctc_beam_lm_abi_version": (cint, []),
            "ts_ctc_beam_lm_launch_config": (cint, [i32, i32, i32, vp, vp, vp]),
            "ts_ctc_beam_lm_workspace_bytes": (i64, [i32, i32, i32, i32]),
            # "ts_ctc_lm*": POINTER of the struct below (each parse makes its own struct class)
            "ts_ctc_beam_lm_search": (cint, [vp, i32, i32, i32, i32, vp, i32, i32, i32, i32, i32, "ts_ctc_lm*", vp, vp, vp, vp, vp, vp, vp, vp]),
        },
        structs={"ts_ctc_lm": [(n, i32) for n in ("n_states", "n_arcs", "start_state", "has_eos")] + [
            (n, vp) for n in ("arc_begin", "arc_class", "arc_next", "arc_factor", "arc_log10", "bo_next", "bo_factor", "bo_log10", "eos_factor", "eos_log10")]},
        out_of_scope=("word-level LMs", "lexicon constraints", "hot-word boosting", "neural LMs")),
    "lora_train": dict(
        names=["ts_lora_abi_version", "ts_lora_fwd", "ts_lora_bwd_workspace", "ts_lora_bwd"],
        version=1,
        signatures={
            "ts_lora_abi_version": (cint, []),
            "ts_lora_fwd": (cint, [vp, i64, i32, vp, vp, i32, i32, f32, vp, i64, vp, vp]),
            "ts_lora_bwd_workspace": (i64, [i64, i32, i32, i32]),
            "ts_lora_bwd": (cint, [vp, i64, vp, vp, i64, i32, i32, i32, f32] + [vp] * 7),
        }),
    "mms": dict(
        names=["ts_mms_abi_version", "ts_mms_attention_fwd", "ts_mms_attn_adapter_fwd"],
        version=1,
        signatures={
            "ts_mms_abi_version": (cint, []),
            "ts_mms_attention_fwd": (cint, [vp, i32, i32, i32, i32, vp, vp, vp]),
            "ts_mms_attn_adapter_fwd": (cint, [vp, i64, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, f32, vp, vp, i32, vp]),
        }),
    "mms_adapter_train": dict(
        names=["ts_mms_adapter_train_abi_version", "ts_mms_attn_adapter_train_fwd", "ts_mms_attn_adapter_train_bwd_workspace",
               "ts_mms_attn_adapter_train_bwd"],
        version=1,
        signatures={
            "ts_mms_adapter_train_abi_version": (cint, []),
            "ts_mms_attn_adapter_train_fwd": (cint, [vp, i64, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp]),
            "ts_mms_attn_adapter_train_bwd_workspace": (i64, [i64, i32, i32]),
            "ts_mms_attn_adapter_train_bwd": (cint, [vp, vp, i64, i32, i32] + [vp] * 13 + [i32, vp]),
        }),
    "mms_train": dict(
        names=["ts_mms_train_abi_version", "ts_mms_attention_train_fwd_workspace", "ts_mms_attention_train_fwd",
               "ts_mms_attention_train_bwd_workspace", "ts_mms_attention_train_bwd"],
        version=1,
        signatures={
            "ts_mms_train_abi_version": (cint, []),
            "ts_mms_attention_train_fwd_workspace": (i64, [i32, i32, i32, i32]),
            "ts_mms_attention_train_bwd_workspace": (i64, [i32, i32, i32, i32]),
            "ts_mms_attention_train_fwd": (cint, [vp, i32, i32, i32, i32, vp, f32, u64, vp, vp, vp, vp]),
            "ts_mms_attention_train_bwd": (cint, [vp, i32, i32, i32, i32, vp, f32, u64, vp, vp, vp, vp, vp, vp, vp]),
        }),
    "posconv_stack_train": dict(
        names=["ts_posconv_stack_train_abi_version", "ts_posconv_stack_conv_workspace", "ts_posconv_stack_conv", "ts_posconv_stack_norm_gelu_fwd",
               "ts_posconv_stack_norm_gelu_bwd_workspace", "ts_posconv_stack_norm_gelu_bwd"],
        version=1,
        signatures={
            "ts_posconv_stack_train_abi_version": (cint, []),
            "ts_posconv_stack_conv_workspace": (i64, [i32, i32, i32, i32]),
            "ts_posconv_stack_conv": (cint, [vp, i32, i32, i32, vp, i32, i32, i32, vp, vp, vp]),
            "ts_posconv_stack_norm_gelu_fwd": (cint, [vp, vp, f32, i64, i32, vp, vp]),
            "ts_posconv_stack_norm_gelu_bwd_workspace": (i64, [i64, i32]),
            "ts_posconv_stack_norm_gelu_bwd": (cint, [vp, vp, vp, f32, i64, i32, vp, vp, vp, vp]),
        }),
    "sew": dict(
        names=["ts_sew_abi_version", "ts_sew_squeeze_workspace_bytes", "ts_sew_squeeze_fwd", "ts_sew_unsqueeze_rows"],
        version=1,
        signatures={
            "ts_sew_abi_version": (cint, []),
            "ts_sew_squeeze_workspace_bytes": (i64, [i32, i32, i32, i32, i32, i32]),
            "ts_sew_squeeze_fwd": (cint, [vp, i32, i32, i32, vp, vp, i32, i32, i32, i32, vp, vp, vp]),
            "ts_sew_unsqueeze_rows": (cint, [vp, i32, i32, i32, i32, i32, vp, vp]),
        }),
    "sew_train": dict(
        names=["ts_sew_train_abi_version", "ts_sew_squeeze_train_supported", "ts_sew_squeeze_train_fwd", "ts_sew_squeeze_dgrad_workspace_bytes",
               "ts_sew_squeeze_dgrad", "ts_sew_squeeze_wgrad_workspace_bytes", "ts_sew_squeeze_wgrad"],
        version=1,
        signatures={
            "ts_sew_squeeze_train_supported": (cint, [i32] * 6),
            "ts_sew_squeeze_train_fwd": (cint, [vp, i32, i32, i32, vp, vp, i32, i32, i32, vp, vp, vp, vp]),
            "ts_sew_squeeze_dgrad": (cint, [vp, vp, i32, i32, i32, vp, i32, i32, i32, vp, vp, vp]),
            "ts_sew_squeeze_wgrad": (cint, [vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp]),
            "ts_sew_squeeze_dgrad_workspace_bytes": (i64, [i32] * 5),
            "ts_sew_squeeze_wgrad_workspace_bytes": (i64, [i32] * 5),
        }),
    "wavlm": dict(
        names=["ts_wavlm_abi_version", "ts_wavlm_rel_bias", "ts_wavlm_attention_workspace_bytes", "ts_wavlm_attention_fwd"],
        version=1,
        argtypes={"ts_wavlm_attention_fwd": [vp, i32, i32, i32, i32, vp, i32, vp, i64, vp, vp, vp, vp, vp, vp, vp]}),
    "wavlm_train": dict(
        names=["ts_wavlm_train_abi_version", "ts_wavlm_gate_fwd", "ts_wavlm_gate_bwd_workspace", "ts_wavlm_gate_bwd",
               "ts_wavlm_attention_train_fwd_workspace", "ts_wavlm_attention_train_fwd", "ts_wavlm_attention_train_bwd_workspace",
               "ts_wavlm_attention_train_bwd", "ts_wavlm_rel_bias_bwd"],
        version=1,
        argtypes={"ts_wavlm_attention_train_bwd": [vp, i32, i32, i32, i32, vp, f32, u64] + [vp] * 11,
                  "ts_wavlm_gate_fwd": [vp, i32, i32, i32, i64] + [vp] * 6},
        restypes={"ts_wavlm_attention_train_bwd_workspace": i64}),
}
STEMS = sorted(COMPANIONS)
HEADERS = [CORE] + [os.path.join(INCLUDE, "thunder_speech_amd", stem + ".h") for stem in STEMS]


def _path(stem):
    return os.path.join(INCLUDE, "thunder_speech_amd", stem + ".h")


def _code(path):
    """The header's text without its comments, both styles (what `read_header` parses)."""
    return re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(path).read(), flags=re.S)


def _declared(path):
    return sorted(set(re.findall(r"\b(ts_[a-z0-9_]+)\s*\(", _code(path))))


def _fields(struct):
    return [(n, t) for n, t in struct._fields_]


def _type_names(signature):
    return signature[0].__name__, [a.__name__ for a in signature[1]]


def _resolve(signature, structs):
    """The table's signature with its struct-pointer placeholders ("<typedef name>*") replaced by POINTER of that parse's struct class."""
    restype, argtypes = signature
    return restype, [ctypes.POINTER(structs[a[:-1]]) if isinstance(a, str) else a for a in argtypes]


@pytest.fixture(scope="module")
def built_library():
    from thunder_speech_amd import build as b
    return b.build(verbose=False)


# ---- each companion against the table ----------------------------------------------------------------------------------------------------------
def test_the_table_and_the_binding_hold_the_same_companions_in_the_same_order():
    from thunder_speech_amd import _lib
    assert list(_lib.COMPANIONS) == STEMS and len(STEMS) == 14
    assert [c.path for c in _lib.COMPANIONS.values()] == HEADERS[1:]


@pytest.mark.parametrize("stem", STEMS)
def test_companion_header_parses_declares_exactly_its_names_and_is_bound_as_parsed(stem):
    from thunder_speech_amd import _lib
    row, bound, path = COMPANIONS[stem], _lib.COMPANIONS[stem], _path(stem)
    assert bound.path == path
    text = open(path).read()
    sigs, structs, defines = _lib.read_header(text)
    # names, three ways: the parse, a plain regex over the text, the table
    assert sorted(sigs) == _declared(path) == sorted(row["names"]) == sorted(bound.signatures)
    assert list(sigs) == list(bound.signatures) and defines == bound.defines
    # the version pair is the header's own: one define, one function, no naming rule
    assert [n for n in defines if n.endswith("ABI_VERSION")] == [bound.version_define]
    assert [n for n in sigs if n.endswith("abi_version")] == [bound.version_function] and sigs[bound.version_function] == (cint, [])
    assert defines[bound.version_define] == bound.abi_version == row["version"]
    # structs: the table's, field by field; a second parse makes classes of its own, equal in everything but identity
    want_structs = row.get("structs", {})
    assert list(structs) == list(bound.structs) == list(want_structs)
    for name, fields in want_structs.items():
        assert _fields(structs[name]) == _fields(bound.structs[name]) == fields
    for name in sigs:
        if any(issubclass(a, ctypes._Pointer) for a in sigs[name][1]):       # a struct pointer: the same type by name, the fields are above
            assert _type_names(bound.signatures[name]) == _type_names(sigs[name]), name
        else:
            assert bound.signatures[name] == sigs[name], name
    # the exact ctypes signatures
    for name, signature in row.get("signatures", {}).items():
        assert sigs[name] == _resolve(signature, structs), name
        assert bound.signatures[name] == _resolve(signature, bound.structs), name
    for name, argtypes in row.get("argtypes", {}).items():
        assert sigs[name][1] == bound.signatures[name][1] == argtypes, name
    for name, restype in row.get("restypes", {}).items():
        assert sigs[name][0] == bound.signatures[name][0] == restype, name
    for phrase in row.get("out_of_scope", ()):
        assert phrase in text                                                 # the header names what is out of scope


@pytest.mark.parametrize("path", HEADERS[1:], ids=STEMS)
def test_companion_headers_use_only_the_types_read_header_maps(path):
    assert not re.search(r"\b(size_t|double)\b", _code(path))


def test_the_lm_struct_is_the_bound_one_and_the_search_without_an_lm_keeps_its_four_names():
    from thunder_speech_amd import _lib
    lm = _lib.COMPANIONS["ctc_beam_lm"]
    assert _lib.CtcLm is lm.structs["ts_ctc_lm"] and _fields(_lib.CtcLm) == COMPANIONS["ctc_beam_lm"]["structs"]["ts_ctc_lm"]
    assert lm.signatures["ts_ctc_beam_lm_search"][1][11] is ctypes.POINTER(_lib.CtcLm)
    assert sorted(_lib.COMPANIONS["ctc_beam"].signatures) == sorted(COMPANIONS["ctc_beam"]["names"]) \
        == [n.replace("_lm", "") for n in sorted(COMPANIONS["ctc_beam_lm"]["names"])]


@pytest.mark.parametrize("text,found", [
    ("int ts_x(int a);\n", "[] and []"),
    ("#define TS_A_ABI_VERSION 1\n#define TS_B_ABI_VERSION 2\nint ts_a_abi_version(void);\n", "['TS_A_ABI_VERSION', 'TS_B_ABI_VERSION'] and ['ts_a_abi_version']"),
    ("#define TS_A_ABI_VERSION 1\nint ts_a_abi_version(void);\nint ts_b_abi_version(void);\n", "['TS_A_ABI_VERSION'] and ['ts_a_abi_version', 'ts_b_abi_version']"),
])
def test_a_header_without_exactly_one_version_pair_is_refused_by_name(text, found, tmp_path):
    from thunder_speech_amd import _lib
    path = tmp_path / "odd.h"
    path.write_text(text)
    with pytest.raises(RuntimeError) as e:
        _lib._read_installed_header(str(path))
    assert str(path) in str(e.value) and found in str(e.value)
    path.write_text("#define TS_Q_ABI_VERSION 3\nint ts_other_abi_version(void);\n")       # the pair needs no common stem
    header = _lib._read_installed_header(str(path))
    assert (header.version_define, header.version_function, header.abi_version) == ("TS_Q_ABI_VERSION", "ts_other_abi_version", 3)


@pytest.mark.parametrize("stem", STEMS)
def test_the_loaded_library_reports_the_version_its_header_declares(stem, built_library):
    from thunder_speech_amd import _lib
    bound = _lib.COMPANIONS[stem]
    assert getattr(_lib.lib(), bound.version_function)() == bound.abi_version == COMPANIONS[stem]["version"]


# ---- the fifteen headers together ----------------------------------------------------------------------------------------------------------------
def test_include_holds_exactly_the_core_header_and_the_fourteen_companions():
    found = sorted(os.path.relpath(os.path.join(d, f), INCLUDE) for d, _, files in os.walk(INCLUDE) for f in files)
    assert found == sorted(["thunder_speech_amd.h"] + [os.path.join("thunder_speech_amd", stem + ".h") for stem in STEMS])
    assert glob.glob(os.path.join(ROOT, "thunder_speech_amd", "**", "*.h"), recursive=True) == []        # no header lives inside the package


def test_no_name_is_declared_by_two_headers():
    from thunder_speech_amd import _lib
    declared = {path: set(_declared(path)) for path in HEADERS}
    for a, b in itertools.combinations(HEADERS, 2):
        assert not declared[a] & declared[b], f"{sorted(declared[a] & declared[b])}: declared in {a} and in {b}"
    tables = [_lib.SIGNATURES] + [c.signatures for c in _lib.COMPANIONS.values()]
    names = [n for table in tables for n in table]
    assert len(names) == len(set(names)) == sum(len(d) for d in declared.values())


def test_the_core_abi_is_unchanged():
    from thunder_speech_amd import _lib
    core = _declared(CORE)
    assert len(core) == 123 and sorted(_lib.SIGNATURES) == core and _lib.EXPORTED_SYMBOLS == list(_lib.SIGNATURES)
    assert _lib.ABI_VERSION == 15 and len(_lib.SIGNATURES) == len(_lib.EXPORTED_SYMBOLS) == 123
    assert _lib.CORE.path == _lib.HEADER == CORE and (_lib.CORE.version_define, _lib.CORE.version_function) == ("TS_ABI_VERSION", "ts_abi_version")


def test_built_library_defines_every_declared_name_of_every_header(built_library):
    nm = subprocess.run(["nm", "-D", "--defined-only", built_library], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for path in HEADERS:
        assert not [s for s in _declared(path) if s not in defined], path
    for stem in STEMS:
        assert set(COMPANIONS[stem]["names"]) <= defined


@pytest.mark.parametrize("header", HEADERS, ids=["core"] + STEMS)
def test_editing_a_header_makes_the_library_stale(header, tmp_path, monkeypatch):
    """build.needs_build() looks at every header of the ABI: one newer than the library asks for a rebuild, an older one does not."""
    from thunder_speech_amd import build as b
    lib = tmp_path / "lib.so"
    lib.write_bytes(b"")
    monkeypatch.setattr(b, "lib_path", lambda: str(lib))
    # only this header counts here: every other dependency is taken out of the comparison
    real = glob.glob
    monkeypatch.setattr(b, "sources", lambda: [])
    monkeypatch.setattr(b.glob, "glob", lambda pat, **kw: [p for p in real(pat, **kw) if p == header])
    mtime = os.path.getmtime(header)
    os.utime(lib, (mtime + 10, mtime + 10))
    assert not b.needs_build()
    os.utime(lib, (mtime - 10, mtime - 10))
    assert b.needs_build()
