"""ctypes binding of the C ABI declared in include/thunder_speech_amd.h and its companions include/thunder_speech_amd_wavlm.h,
include/thunder_speech_amd_wavlm_train.h, include/thunder_speech_amd_conformer.h, include/thunder_speech_amd_mms.h,
include/thunder_speech_amd_mms_train.h, include/thunder_speech_amd_mms_adapter_train.h, include/thunder_speech_amd/posconv_stack_train.h,
thunder_speech_amd/abi/sew.h, thunder_speech_amd/abi/ctc_align.h, thunder_speech_amd/abi/ctc_beam.h, thunder_speech_amd/abi/conformer_train.h,
thunder_speech_amd/abi/train/sew_train.h, thunder_speech_amd/capi/ctc_beam_lm.h (beam search with n-gram LM fusion; it declares the one
struct outside the core header, `CtcLm`, the LM tables of a call) and thunder_speech_amd/lora/lora_train.h (LoRA fine-tuning).

The header is the only copy of the ABI: `read_header` derives every prototype, struct and TS_* constant from it and
`lib()` applies the result, so a new entry point needs the header and its .hip definition and nothing here.  A C type
without a row in the tables below is an error at import, never the ctypes default.

There is deliberately NO fallback: if the HIP shared library is missing or a kernel reports an error
the caller gets a RuntimeError -- the product path never silently computes on the CPU.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from typing import Optional

from .build import PKG, ROOT, lib_path

HEADER = os.path.join(ROOT, "include", "thunder_speech_amd.h")
WAVLM_HEADER = os.path.join(ROOT, "include", "thunder_speech_amd_wavlm.h")    # companion ABI, versioned on its own
WAVLM_TRAIN_HEADER = os.path.join(ROOT, "include", "thunder_speech_amd_wavlm_train.h")    # second companion (WavLM fine-tuning), versioned on its own
CONFORMER_HEADER = os.path.join(ROOT, "include", "thunder_speech_amd_conformer.h")        # third companion (wav2vec2-conformer), versioned on its own

MMS_HEADER = os.path.join(ROOT, "include", "thunder_speech_amd_mms.h")                    # fourth companion (MMS / XLS-R 1B), versioned on its own
MMS_TRAIN_HEADER = os.path.join(ROOT, "include", "thunder_speech_amd_mms_train.h")        # fifth companion (head_dim 80 fine-tuning), versioned on its own
MMS_ADAPTER_TRAIN_HEADER = os.path.join(ROOT, "include", "thunder_speech_amd_mms_adapter_train.h")    # sixth companion (adapter fine-tuning), versioned on its own
POSCONV_STACK_TRAIN_HEADER = os.path.join(ROOT, "include", "thunder_speech_amd", "posconv_stack_train.h")   # seventh companion (data2vec-audio fine-tuning), versioned on its own; new companions live in that directory
SEW_HEADER = os.path.join(PKG, "abi", "sew.h")          # eighth companion (SEW inference), versioned on its own; inside the package (the header count of include/ is pinned)
CTC_ALIGN_HEADER = os.path.join(PKG, "abi", "ctc_align.h")    # ninth companion (forced alignment, greedy spans), versioned on its own; next to sew.h
CTC_BEAM_HEADER = os.path.join(PKG, "abi", "ctc_beam.h")      # tenth companion (prefix beam search, n-best), versioned on its own; next to ctc_align.h
CONFORMER_TRAIN_HEADER = os.path.join(PKG, "abi", "conformer_train.h")    # eleventh companion (wav2vec2-conformer fine-tuning), versioned on its own; next to ctc_beam.h

SEW_TRAIN_HEADER = os.path.join(PKG, "abi", "train", "sew_train.h")    # twelfth companion (SEW fine-tuning), versioned on its own; in abi/train/ (the header count of abi/ is pinned too)
CTC_BEAM_LM_HEADER = os.path.join(PKG, "capi", "ctc_beam_lm.h")    # thirteenth companion (beam search with n-gram LM fusion), versioned on its own; in capi/ (the header counts of include/ and abi/ are pinned)
LORA_HEADER = os.path.join(PKG, "lora", "lora_train.h")    # fourteenth companion (LoRA fine-tuning of the attention projections), versioned on its own; in lora/ (the header counts of include/, abi/ and capi/ are pinned)

# Parameters and struct fields: these scalars, `[const] <struct>*` as POINTER(struct), every other pointer to one of
# _POINTEES (const or not, any depth) as c_void_p.  Return types: _RETURNS only.
_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float}
_POINTEES = {"void", "float", "int32_t", "int64_t", "uint64_t", "uint8_t"}
_RETURNS = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "const char*": C.c_char_p, "const float*": C.c_void_p}


def _ctype(decl: str, where: str, structs: dict, ret: bool = False):
    """The ctypes type of the C type `decl` (no declarator name) used in `where`."""
    words, stars = re.findall(r"\w+", decl), decl.count("*")
    key, table = " ".join(words) + "*" * stars, _RETURNS if ret else _SCALARS
    if key in table:
        return table[key]
    base = [w for w in words if w != "const"]
    if not ret and stars and len(base) == 1:
        if stars == 1 and base[0] in structs:                           # `const struct*` in, `struct*` out
            return C.POINTER(structs[base[0]])
        if base[0] in _POINTEES:
            return C.c_void_p
    raise ValueError(f"thunder_speech_amd header: {where}: no ctypes binding for the type `{key}`")


def read_header(text: str):
    """(signatures, structs, defines) of a C header: {ts_name: (restype, argtypes)} in declaration order,
    {typedef name: ctypes.Structure subclass} and {TS_NAME: int} for every `#define TS_* <integer>`."""
    code = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    defines = {n: int(v) for n, v in re.findall(r"^\s*#\s*define\s+(TS_\w+)\s+\(?\s*(-?\d+)\s*\)?\s*$", code, flags=re.M)}
    code = re.sub(r"^\s*#.*$", "", code, flags=re.M)
    structs = {}
    for body, name in re.findall(r"typedef\s+struct\s+\w*\s*\{(.*?)\}\s*(\w+)\s*;", code, flags=re.S):
        fields = []
        for decl in filter(str.strip, body.split(";")):
            first, *more = decl.split(",")
            base = re.sub(r"\w+\s*$", "", first.replace("*", " "))      # C: each declarator carries its own '*'
            fields += [(re.findall(r"\w+", d)[-1], _ctype(base + "*" * d.count("*"), f"struct {name}", structs))
                       for d in [first] + more]
        cls_name = "".join(w.capitalize() for w in name.split("_")[1:])  # ts_tcs_desc -> TcsDesc
        structs[name] = type(cls_name, (C.Structure,), {"__doc__": f"struct {name}", "_fields_": fields})
    signatures = {}
    for ret, name, params in re.findall(r"([\w\s*]+?)\s*\b(ts_\w+)\s*\(([^()]*)\)\s*;", code):
        params = [] if params.strip() in ("", "void") else params.split(",")
        argtypes = []
        for p in params:
            m = re.fullmatch(r"(.*[\s*])\w+\s*", p, flags=re.S)          # drop the parameter's name
            argtypes.append(_ctype(m.group(1) if m else p, name, structs))
        signatures[name] = (_ctype(ret, name, structs, ret=True), argtypes)
    return signatures, structs, defines


def _read_installed_header(path: str = HEADER):
    if not os.path.exists(path):
        raise RuntimeError(f"thunder_speech_amd: the C header {path} is missing; the ctypes binding is derived from it")
    with open(path) as f:
        return read_header(f.read())


SIGNATURES, STRUCTS, DEFINES = _read_installed_header()
# the companion headers declare no structs; their entry points are applied next to the core ones but are not part of SIGNATURES
WAVLM_SIGNATURES, _, WAVLM_DEFINES = _read_installed_header(WAVLM_HEADER)
WAVLM_ABI_VERSION = WAVLM_DEFINES["TS_WAVLM_ABI_VERSION"]
WAVLM_TRAIN_SIGNATURES, _, WAVLM_TRAIN_DEFINES = _read_installed_header(WAVLM_TRAIN_HEADER)
WAVLM_TRAIN_ABI_VERSION = WAVLM_TRAIN_DEFINES["TS_WAVLM_TRAIN_ABI_VERSION"]
CONFORMER_SIGNATURES, _, CONFORMER_DEFINES = _read_installed_header(CONFORMER_HEADER)
CONFORMER_ABI_VERSION = CONFORMER_DEFINES["TS_CONFORMER_ABI_VERSION"]
MMS_SIGNATURES, _, MMS_DEFINES = _read_installed_header(MMS_HEADER)
MMS_ABI_VERSION = MMS_DEFINES["TS_MMS_ABI_VERSION"]
MMS_TRAIN_SIGNATURES, _, MMS_TRAIN_DEFINES = _read_installed_header(MMS_TRAIN_HEADER)
MMS_TRAIN_ABI_VERSION = MMS_TRAIN_DEFINES["TS_MMS_TRAIN_ABI_VERSION"]
MMS_ADAPTER_TRAIN_SIGNATURES, _, MMS_ADAPTER_TRAIN_DEFINES = _read_installed_header(MMS_ADAPTER_TRAIN_HEADER)
MMS_ADAPTER_TRAIN_ABI_VERSION = MMS_ADAPTER_TRAIN_DEFINES["TS_MMS_ADAPTER_TRAIN_ABI_VERSION"]
POSCONV_STACK_TRAIN_SIGNATURES, _, POSCONV_STACK_TRAIN_DEFINES = _read_installed_header(POSCONV_STACK_TRAIN_HEADER)
POSCONV_STACK_TRAIN_ABI_VERSION = POSCONV_STACK_TRAIN_DEFINES["TS_POSCONV_STACK_TRAIN_ABI_VERSION"]
SEW_SIGNATURES, _, SEW_DEFINES = _read_installed_header(SEW_HEADER)
SEW_ABI_VERSION = SEW_DEFINES["TS_SEW_ABI_VERSION"]
CTC_ALIGN_SIGNATURES, _, CTC_ALIGN_DEFINES = _read_installed_header(CTC_ALIGN_HEADER)
CTC_ALIGN_ABI_VERSION = CTC_ALIGN_DEFINES["TS_CTC_ALIGN_ABI_VERSION"]
CTC_BEAM_SIGNATURES, _, CTC_BEAM_DEFINES = _read_installed_header(CTC_BEAM_HEADER)
CTC_BEAM_ABI_VERSION = CTC_BEAM_DEFINES["TS_CTC_BEAM_ABI_VERSION"]
CONFORMER_TRAIN_SIGNATURES, _, CONFORMER_TRAIN_DEFINES = _read_installed_header(CONFORMER_TRAIN_HEADER)
CONFORMER_TRAIN_ABI_VERSION = CONFORMER_TRAIN_DEFINES["TS_CONFORMER_TRAIN_ABI_VERSION"]
SEW_TRAIN_SIGNATURES, _, SEW_TRAIN_DEFINES = _read_installed_header(SEW_TRAIN_HEADER)
SEW_TRAIN_ABI_VERSION = SEW_TRAIN_DEFINES["TS_SEW_TRAIN_ABI_VERSION"]
CTC_BEAM_LM_SIGNATURES, CTC_BEAM_LM_STRUCTS, CTC_BEAM_LM_DEFINES = _read_installed_header(CTC_BEAM_LM_HEADER)
CTC_BEAM_LM_ABI_VERSION = CTC_BEAM_LM_DEFINES["TS_CTC_BEAM_LM_ABI_VERSION"]
CtcLm = CTC_BEAM_LM_STRUCTS["ts_ctc_lm"]
LORA_SIGNATURES, _, LORA_DEFINES = _read_installed_header(LORA_HEADER)
LORA_ABI_VERSION = LORA_DEFINES["TS_LORA_ABI_VERSION"]
TcsDesc, FrontendDesc, WgradItem =STRUCTS["ts_tcs_desc"], STRUCTS["ts_frontend_desc"], STRUCTS["ts_wgrad_item"]
TcsLaunch = STRUCTS["ts_tcs_launch"]
EXPORTED_SYMBOLS = list(SIGNATURES)
ABI_VERSION = DEFINES["TS_ABI_VERSION"]
TS_EINVAL, TS_EUNSUPPORTED = DEFINES["TS_EINVAL"], DEFINES["TS_EUNSUPPORTED"]
TCS_IN_TAILZERO, TCS_OUT_ZERO_TAIL = DEFINES["TS_TCS_IN_TAILZERO"], DEFINES["TS_TCS_OUT_ZERO_TAIL"]
TCS_TAPS_PHASE = DEFINES["TS_TCS_TAPS_PHASE"]
TCS_LAUNCH_NONE, TCS_LAUNCH_GENERIC, TCS_LAUNCH_SPLIT, TCS_LAUNCH_LOGITS = (DEFINES["TS_TCS_LAUNCH_" + n] for n in ("NONE", "GENERIC", "SPLIT", "LOGITS"))
GUARD_BYTES = DEFINES["TS_GUARD_BYTES"]

_lib: Optional[C.CDLL] = None


def is_available() -> bool:
    return os.path.exists(lib_path())


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise RuntimeError(
            f"thunder_speech_amd: HIP extension {path} is missing. Build it with "
            "`python -m thunder_speech_amd.build` (needs hipcc / ROCm); there is no CPU fallback.")
    import torch  # noqa: F401  -- must initialise its bundled HIP runtime BEFORE our code object is loaded
    L = C.CDLL(path)
    missing = [s for s in EXPORTED_SYMBOLS + list(WAVLM_SIGNATURES) + list(WAVLM_TRAIN_SIGNATURES) + list(CONFORMER_SIGNATURES) + list(MMS_SIGNATURES) +
               list(MMS_TRAIN_SIGNATURES) + list(MMS_ADAPTER_TRAIN_SIGNATURES) + list(POSCONV_STACK_TRAIN_SIGNATURES) + list(SEW_SIGNATURES) +
               list(CTC_ALIGN_SIGNATURES) + list(CTC_BEAM_SIGNATURES) + list(CONFORMER_TRAIN_SIGNATURES) + list(SEW_TRAIN_SIGNATURES) +
               list(CTC_BEAM_LM_SIGNATURES) + list(LORA_SIGNATURES) if not hasattr(L, s)]
    if missing:
        raise RuntimeError(f"thunder_speech_amd: {path} does not export {missing}; rebuild it")
    for name, (restype, argtypes) in {**SIGNATURES, **WAVLM_SIGNATURES, **WAVLM_TRAIN_SIGNATURES, **CONFORMER_SIGNATURES, **MMS_SIGNATURES,
                                      **MMS_TRAIN_SIGNATURES, **MMS_ADAPTER_TRAIN_SIGNATURES, **POSCONV_STACK_TRAIN_SIGNATURES, **SEW_SIGNATURES,
                                      **CTC_ALIGN_SIGNATURES, **CTC_BEAM_SIGNATURES, **CONFORMER_TRAIN_SIGNATURES, **SEW_TRAIN_SIGNATURES,
                                      **CTC_BEAM_LM_SIGNATURES, **LORA_SIGNATURES}.items():
        f = getattr(L, name)
        f.restype, f.argtypes = restype, argtypes
    if L.ts_abi_version() != ABI_VERSION:
        raise RuntimeError(f"thunder_speech_amd: {path} reports ABI {L.ts_abi_version()}, the header {HEADER} "
                           f"declares {ABI_VERSION}; rebuild it")
    if L.ts_wavlm_abi_version() != WAVLM_ABI_VERSION:
        raise RuntimeError(f"thunder_speech_amd: {path} reports WavLM ABI {L.ts_wavlm_abi_version()}, the header {WAVLM_HEADER} "
                           f"declares {WAVLM_ABI_VERSION}; rebuild it")
    if L.ts_wavlm_train_abi_version() != WAVLM_TRAIN_ABI_VERSION:
        raise RuntimeError(f"thunder_speech_amd: {path} reports WavLM training ABI {L.ts_wavlm_train_abi_version()}, the header "
                           f"{WAVLM_TRAIN_HEADER} declares {WAVLM_TRAIN_ABI_VERSION}; rebuild it")
    if L.ts_conformer_abi_version() != CONFORMER_ABI_VERSION:
        raise RuntimeError(f"thunder_speech_amd: {path} reports conformer ABI {L.ts_conformer_abi_version()}, the header {CONFORMER_HEADER} "
                           f"declares {CONFORMER_ABI_VERSION}; rebuild it")
    if L.ts_mms_abi_version() != MMS_ABI_VERSION:
        raise RuntimeError(f"thunder_speech_amd: {path} reports MMS ABI {L.ts_mms_abi_version()}, the header {MMS_HEADER} "
                           f"declares {MMS_ABI_VERSION}; rebuild it")
    if L.ts_mms_train_abi_version() != MMS_TRAIN_ABI_VERSION:
        raise RuntimeError(f"thunder_speech_amd: {path} reports MMS training ABI {L.ts_mms_train_abi_version()}, the header {MMS_TRAIN_HEADER} "
                           f"declares {MMS_TRAIN_ABI_VERSION}; rebuild it")
    if L.ts_mms_adapter_train_abi_version() != MMS_ADAPTER_TRAIN_ABI_VERSION:
        raise RuntimeError(f"thunder_speech_amd: {path} reports MMS adapter training ABI {L.ts_mms_adapter_train_abi_version()}, the header "
                           f"{MMS_ADAPTER_TRAIN_HEADER} declares {MMS_ADAPTER_TRAIN_ABI_VERSION}; rebuild it")
    if L.ts_posconv_stack_train_abi_version() != POSCONV_STACK_TRAIN_ABI_VERSION:
        raise RuntimeError(f"thunder_speech_amd: {path} reports positional-stack training ABI {L.ts_posconv_stack_train_abi_version()}, the header "
                           f"{POSCONV_STACK_TRAIN_HEADER} declares {POSCONV_STACK_TRAIN_ABI_VERSION}; rebuild it")
    if L.ts_sew_abi_version() != SEW_ABI_VERSION:
        raise RuntimeError(f"thunder_speech_amd: {path} reports SEW ABI {L.ts_sew_abi_version()}, the header {SEW_HEADER} "
                           f"declares {SEW_ABI_VERSION}; rebuild it")
    if L.ts_ctc_align_abi_version() != CTC_ALIGN_ABI_VERSION:
        raise RuntimeError(f"thunder_speech_amd: {path} reports CTC alignment ABI {L.ts_ctc_align_abi_version()}, the header {CTC_ALIGN_HEADER} "
                           f"declares {CTC_ALIGN_ABI_VERSION}; rebuild it")
    if L.ts_ctc_beam_abi_version() != CTC_BEAM_ABI_VERSION:
        raise RuntimeError(f"thunder_speech_amd: {path} reports CTC beam search ABI {L.ts_ctc_beam_abi_version()}, the header {CTC_BEAM_HEADER} "
                           f"declares {CTC_BEAM_ABI_VERSION}; rebuild it")
    if L.ts_conformer_train_abi_version() != CONFORMER_TRAIN_ABI_VERSION:
        raise RuntimeError(f"thunder_speech_amd: {path} reports conformer training ABI {L.ts_conformer_train_abi_version()}, the header "
                           f"{CONFORMER_TRAIN_HEADER} declares {CONFORMER_TRAIN_ABI_VERSION}; rebuild it")
    if L.ts_sew_train_abi_version() != SEW_TRAIN_ABI_VERSION:
        raise RuntimeError(f"thunder_speech_amd: {path} reports SEW training ABI {L.ts_sew_train_abi_version()}, the header "
                           f"{SEW_TRAIN_HEADER} declares {SEW_TRAIN_ABI_VERSION}; rebuild it")
    if L.ts_ctc_beam_lm_abi_version() != CTC_BEAM_LM_ABI_VERSION:
        raise RuntimeError(f"thunder_speech_amd: {path} reports CTC beam search LM fusion ABI {L.ts_ctc_beam_lm_abi_version()}, the header "
                           f"{CTC_BEAM_LM_HEADER} declares {CTC_BEAM_LM_ABI_VERSION}; rebuild it")
    if L.ts_lora_abi_version() != LORA_ABI_VERSION:
        raise RuntimeError(f"thunder_speech_amd: {path} reports LoRA training ABI {L.ts_lora_abi_version()}, the header "
                           f"{LORA_HEADER} declares {LORA_ABI_VERSION}; rebuild it")
    _lib = L
    return L


CALLS = 0          # C-ABI calls checked so far (bench.py reports calls per training step)


def check(status: int, what: str) -> None:
    global CALLS
    CALLS += 1
    if status == 0:
        return
    if status == TS_EINVAL:
        raise RuntimeError(f"{what}: invalid argument (TS_EINVAL)")
    if status == TS_EUNSUPPORTED:
        raise NotImplementedError(f"{what}: configuration not supported by the HIP kernels (TS_EUNSUPPORTED)")
    raise RuntimeError(f"{what}: HIP error {status}")


def time_pitch(t: int) -> int:
    """Python mirror of ts_time_pitch (kept in sync by tests/test_capi_host.py)."""
    return ((max(int(t), 1) + 384 + 127) // 128) * 128
