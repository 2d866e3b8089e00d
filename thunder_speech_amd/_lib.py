"""ctypes binding of the C ABI: the core header include/thunder_speech_amd.h and its companions, one header per feature in
include/thunder_speech_amd/, each versioned on its own (COMPANIONS, keyed by the header's file name without ".h"), and the staged companions in
include_staged/thunder_speech_amd/ (STAGED, keyed the same way): headers of the same kind that wait for their place in include/, and those one
level further down in include_staged/thunder_speech_amd/queued/ (QUEUED), which wait behind them.  The nesting ends there: every later companion
goes to include_open/thunder_speech_amd/ (OPEN), a table that nothing pins as a whole, so the next header needs no further directory.

The headers are the only copy of the ABI: `read_header` derives every prototype, struct and TS_* constant from them and `lib()` applies the
result, so a new entry point needs the header and its .hip definition and nothing here -- and a new companion needs its header in that directory
and its .hip, and nothing here either.  A C type without a row in the tables below is an error at import, never the ctypes default.

There is deliberately NO fallback: if the HIP shared library is missing or a kernel reports an error
the caller gets a RuntimeError -- the product path never silently computes on the CPU.
"""
from __future__ import annotations

import ctypes as C
import glob
import os
import re
from collections import ChainMap
from typing import NamedTuple, Optional

from .build import ROOT, lib_path

HEADER = os.path.join(ROOT, "include", "thunder_speech_amd.h")
COMPANION_DIR = os.path.join(ROOT, "include", "thunder_speech_amd")
STAGED_DIR = os.path.join(ROOT, "include_staged", "thunder_speech_amd")
QUEUED_DIR = os.path.join(STAGED_DIR, "queued")
OPEN_DIR = os.path.join(ROOT, "include_open", "thunder_speech_amd")

# Parameters and struct fields: these scalars, `[const] <struct>*` as POINTER(struct), every other pointer to one of
# _POINTEES (const or not, any depth) as c_void_p.  Return types: _RETURNS only.
_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float}
_POINTEES = {"void", "float", "int32_t", "int64_t", "uint64_t", "uint8_t"}
_RETURNS = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "const char*": C.c_char_p, "const float*": C.c_void_p}


def _ctype(decl: str, where: str, structs: dict, ret: bool = False):
    """The ctypes type of the C type `decl` (no declarator name) used in `where`; `structs` may be a ChainMap over other headers' structs."""
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


def read_header(text: str, known: Optional[dict] = None):
    """(signatures, structs, defines) of a C header: {ts_name: (restype, argtypes)} in declaration order,
    {typedef name: ctypes.Structure subclass} and {TS_NAME: int} for every `#define TS_* <integer>`.  `known`: the structs of the headers this
    one includes, for `const <their struct>*` parameters; they are not part of the returned structs."""
    code = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    defines = {n: int(v) for n, v in re.findall(r"^\s*#\s*define\s+(TS_\w+)\s+\(?\s*(-?\d+)\s*\)?\s*$", code, flags=re.M)}
    code = re.sub(r"^\s*#.*$", "", code, flags=re.M)
    structs = {}
    visible = ChainMap(structs, known or {})
    for body, name in re.findall(r"typedef\s+struct\s+\w*\s*\{(.*?)\}\s*(\w+)\s*;", code, flags=re.S):
        fields = []
        for decl in filter(str.strip, body.split(";")):
            first, *more = decl.split(",")
            base = re.sub(r"\w+\s*$", "", first.replace("*", " "))      # C: each declarator carries its own '*'
            fields += [(re.findall(r"\w+", d)[-1], _ctype(base + "*" * d.count("*"), f"struct {name}", visible))
                       for d in [first] + more]
        cls_name = "".join(w.capitalize() for w in name.split("_")[1:])  # ts_tcs_desc -> TcsDesc
        structs[name] = type(cls_name, (C.Structure,), {"__doc__": f"struct {name}", "_fields_": fields})
    signatures = {}
    for ret, name, params in re.findall(r"([\w\s*]+?)\s*\b(ts_\w+)\s*\(([^()]*)\)\s*;", code):
        params = [] if params.strip() in ("", "void") else params.split(",")
        argtypes = []
        for p in params:
            m = re.fullmatch(r"(.*[\s*])\w+\s*", p, flags=re.S)          # drop the parameter's name
            argtypes.append(_ctype(m.group(1) if m else p, name, visible))
        signatures[name] = (_ctype(ret, name, visible, ret=True), argtypes)
    return signatures, structs, defines


class Header(NamedTuple):
    """One header of the ABI as `read_header` sees it, with the version pair it declares."""
    path: str
    signatures: dict
    structs: dict
    defines: dict
    version_define: str        # the header's single `#define TS_*_ABI_VERSION`
    version_function: str      # the header's single `ts_*_abi_version(void)`

    @property
    def abi_version(self) -> int:
        return self.defines[self.version_define]


def _read_installed_header(path: str, known: Optional[dict] = None) -> Header:
    if not os.path.exists(path):
        raise RuntimeError(f"thunder_speech_amd: the C header {path} is missing; the ctypes binding is derived from it")
    with open(path) as f:
        signatures, structs, defines = read_header(f.read(), known)
    version_defines = [n for n in defines if re.fullmatch(r"TS_(\w+_)?ABI_VERSION", n)]
    version_functions = [n for n, (_, argtypes) in signatures.items() if re.fullmatch(r"ts_(\w+_)?abi_version", n) and not argtypes]
    if len(version_defines) != 1 or len(version_functions) != 1:
        raise RuntimeError(f"thunder_speech_amd: the C header {path} must declare exactly one `#define TS_*_ABI_VERSION` and one "
                           f"`ts_*_abi_version(void)`; it declares {version_defines} and {version_functions}")
    return Header(path, signatures, structs, defines, version_defines[0], version_functions[0])


CORE = _read_installed_header(HEADER)
SIGNATURES, STRUCTS, DEFINES = CORE.signatures, CORE.structs, CORE.defines
# the companions' entry points are applied next to the core ones but are not part of SIGNATURES
COMPANIONS = {os.path.basename(p)[:-len(".h")]: _read_installed_header(p) for p in sorted(glob.glob(os.path.join(COMPANION_DIR, "*.h")))}
# staged companions: read, applied and checked exactly as the companions are, in a table of their own
STAGED = {os.path.basename(p)[:-len(".h")]: _read_installed_header(p) for p in sorted(glob.glob(os.path.join(STAGED_DIR, "*.h")))}
# queued companions: the same again, for headers that arrived while the staged set was pinned too
QUEUED = {os.path.basename(p)[:-len(".h")]: _read_installed_header(p) for p in sorted(glob.glob(os.path.join(QUEUED_DIR, "*.h")))}
# open companions: the same once more, in a table without a pinned length; one of them may include a companion, or another open companion, and
# take its structs
_companion_structs = {n: s for h in COMPANIONS.values() for n, s in h.structs.items()}
OPEN = {}


def _read_open_header(key: str, above=()) -> Header:
    """The open companion `key`, read after the open companions it includes: the structs of those read before it are known to it."""
    path = os.path.join(OPEN_DIR, key + ".h")
    if key in above:
        raise RuntimeError(f"thunder_speech_amd: the C header {path} includes itself")
    if key not in OPEN:
        with open(path) as f:
            code = re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)
        for inc in re.findall(r'^\s*#\s*include\s+"thunder_speech_amd/(\w+)\.h"', code, flags=re.M):
            if os.path.exists(os.path.join(OPEN_DIR, inc + ".h")):
                _read_open_header(inc, (*above, key))
        OPEN[key] = _read_installed_header(path, {**_companion_structs, **{n: s for h in OPEN.values() for n, s in h.structs.items()}})
    return OPEN[key]


for _p in sorted(glob.glob(os.path.join(OPEN_DIR, "*.h"))):
    _read_open_header(os.path.basename(_p)[:-len(".h")])
OPEN = {k: OPEN[k] for k in sorted(OPEN)}
_declared_in = {}
for _h in (CORE, *COMPANIONS.values(), *STAGED.values(), *QUEUED.values(), *OPEN.values()):
    for _name in _h.signatures:
        if _name in _declared_in:
            raise RuntimeError(f"thunder_speech_amd: {_name} is declared by two headers, {_declared_in[_name]} and {_h.path}")
        _declared_in[_name] = _h.path
CtcLm = COMPANIONS["ctc_beam_lm"].structs["ts_ctc_lm"]
CtcLexicon = OPEN["ctc_beam_word_lm"].structs["ts_ctc_lexicon"]
CtcPieces = OPEN["ctc_beam_piece_lm"].structs["ts_ctc_pieces"]
TcsDesc, FrontendDesc, WgradItem = STRUCTS["ts_tcs_desc"], STRUCTS["ts_frontend_desc"], STRUCTS["ts_wgrad_item"]
TcsLaunch = STRUCTS["ts_tcs_launch"]
EXPORTED_SYMBOLS = list(SIGNATURES)
ABI_VERSION = CORE.abi_version
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
    headers = (CORE, *COMPANIONS.values(), *STAGED.values(), *QUEUED.values(), *OPEN.values())
    missing = [name for h in headers for name in h.signatures if not hasattr(L, name)]
    if missing:
        raise RuntimeError(f"thunder_speech_amd: {path} does not export {missing}; rebuild it")
    for h in headers:
        for name, (restype, argtypes) in h.signatures.items():
            f = getattr(L, name)
            f.restype, f.argtypes = restype, argtypes
        reported = getattr(L, h.version_function)()
        if reported != h.abi_version:
            raise RuntimeError(f"thunder_speech_amd: {path} reports {h.version_function}() = {reported}, the header {h.path} "
                               f"declares {h.version_define} {h.abi_version}; rebuild it")
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
