"""The fused QuartzNet head on the CPU: the open companion header include_open/thunder_speech_amd/qn_head.h through `_lib.OPEN` and the built library,
the argument checks of ts_qn_head_fwd that return before any device call, and the decoder-weight packer plan.pack_head_wd against a numpy
restatement of the fragment order (tests/test_gpu_qn_head.py has the kernel itself)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ts_qn_head_abi_version", "ts_qn_head_launches", "ts_qn_head_fwd"]
vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64


def test_the_header_is_bound_through_the_open_table_and_declares_exactly_its_names():
    from thunder_speech_amd import _lib
    from thunder_speech_amd import build as b
    assert "qn_head" in _lib.OPEN
    h = _lib.OPEN["qn_head"]
    assert h.path == os.path.join(ROOT, "include_open", "thunder_speech_amd", "qn_head.h") and h.path in b.header_deps()
    assert (h.version_define, h.version_function, h.abi_version) == ("TS_QN_HEAD_ABI_VERSION", "ts_qn_head_abi_version", 1)
    code = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(h.path).read(), flags=re.S)
    assert sorted(h.signatures) == sorted(set(re.findall(r"\b(ts_[a-z0-9_]+)\s*\(", code))) == sorted(NAMES)
    assert h.signatures["ts_qn_head_launches"] == (i64, [])
    assert h.signatures["ts_qn_head_fwd"] == (ctypes.c_int, [vp] * 7 + [i32] * 10 + [vp])
    assert {k: v for k, v in h.defines.items() if k != "TS_QN_HEAD_ABI_VERSION"} == {
        "TS_QN_HEAD_TILE": 96, "TS_QN_HEAD_V_MAX": 32, "TS_QN_HEAD_HIDDEN_STEP": 512, "TS_QN_HEAD_HIDDEN_MAX": 4096, "TS_QN_HEAD_CIN_MAX": 512}
    assert not h.structs
    others = [_lib.CORE, *_lib.COMPANIONS.values(), *_lib.STAGED.values(), *_lib.QUEUED.values(), *(o for k, o in _lib.OPEN.items() if k != "qn_head")]
    assert not [n for o in others for n in o.signatures if n in NAMES]
    assert "qn_head.hip" in {os.path.basename(p) for p in b.sources()}


def test_the_library_exports_every_prototype_and_reports_the_headers_version():
    from thunder_speech_amd import _lib
    from thunder_speech_amd import build as b
    nm = subprocess.run(["nm", "-D", "--defined-only", b.build(verbose=False)], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert not [n for n in NAMES if n not in defined]
    assert _lib.lib().ts_qn_head_abi_version() == _lib.OPEN["qn_head"].abi_version == 1


def _cases():
    """Calls that return before any device call.  Pointers are made-up addresses (never dereferenced on these paths): A is 16-byte aligned."""
    A, E, U = 0x10000, -1, -2
    f = lambda x=A, ln=A, w17=A, b17=A, wd=A, bd=A, y=A, b=2, c_in=512, hidden=1024, v=29, t=100, pin=512, pout=512, k=1, s=1, res=0: (
        x, ln, w17, b17, wd, bd, y, b, c_in, hidden, v, t, pin, pout, k, s, res, None)
    return [
        (f(x=0), E), (f(w17=0), E), (f(b17=0), E), (f(wd=0), E), (f(bd=0), E), (f(y=0), E),
        (f(b=0), E), (f(c_in=0), E), (f(hidden=0), E), (f(v=0), E), (f(t=0), E), (f(b=-1), E),
        (f(v=33), U), (f(v=1024), U),
        (f(c_in=32), U), (f(c_in=96), U), (f(c_in=576), U), (f(c_in=1024), U),
        (f(hidden=256), U), (f(hidden=768), U), (f(hidden=1000), U), (f(hidden=4608), U),
        (f(k=3), U), (f(s=2), U), (f(res=512), U),
        (f(t=100, pin=191), U),              # rows not readable to the end of the second tile (192 frames)
        (f(t=100, pin=100), U), (f(pin=196), U),          # ... and a pitch that is no multiple of 8
        (f(t=100, pout=99), U),
        (f(pin=2097152), U),                 # a clip of 512 x 2^21 bf16 is 2^31 bytes: beyond the kernel's 32-bit offsets
        (f(x=A + 8), U), (f(w17=A + 8), U), (f(wd=A + 2), U), (f(b17=A + 4), U), (f(bd=A + 2), U), (f(y=A + 2), U), (f(ln=A + 2), U),
    ]


@pytest.mark.parametrize("args,want", _cases())
def test_the_entry_point_refuses_before_any_launch(args, want):
    from thunder_speech_amd import _lib
    assert (_lib.TS_EINVAL, _lib.TS_EUNSUPPORTED) == (-1, -2)
    L = _lib.lib()
    n0 = L.ts_qn_head_launches()
    assert L.ts_qn_head_fwd(*args) == want
    assert L.ts_qn_head_launches() == n0


@pytest.mark.parametrize("v,hidden", [(29, 1024), (32, 512), (1, 64), (17, 192)])
def test_pack_head_wd_against_the_fragment_order(v, hidden):
    """Fragment (g, p, vt), lane l, element e = Wd[16 vt + (l & 15)][64 g + 16 (2 p + (e >> 2)) + 4 (l >> 4) + (e & 3)] rounded to bf16, 0 from row v
    on -- element by element in numpy, from the header's sentence alone."""
    from thunder_speech_amd import plan
    rng = np.random.Generator(np.random.PCG64(v * 10000 + hidden))
    w = rng.standard_normal((v, hidden)).astype(np.float32)
    got = plan.pack_head_wd(torch.from_numpy(w))
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (hidden // 64, 2, 2, 64, 8) and got.is_contiguous()
    wb = np.zeros((32, hidden), dtype=np.float32)
    wb[:v] = torch.from_numpy(w).to(torch.bfloat16).float().numpy()
    want = np.empty((hidden // 64, 2, 2, 64, 8), dtype=np.float32)
    for g in range(hidden // 64):
        for p in range(2):
            for vt in range(2):
                for l in range(64):
                    for e in range(8):
                        want[g, p, vt, l, e] = wb[16 * vt + (l & 15), 64 * g + 16 * (2 * p + (e >> 2)) + 4 * (l >> 4) + (e & 3)]
    assert np.array_equal(got.float().numpy(), want)
    # every weight appears exactly once
    assert np.isclose(np.abs(want).sum(), np.abs(wb).sum(), rtol=1e-5)


def test_pack_head_wd_refuses_what_the_kernel_cannot_take():
    from thunder_speech_amd import plan
    with pytest.raises(ValueError):
        plan.pack_head_wd(torch.zeros(33, 1024))
    with pytest.raises(ValueError):
        plan.pack_head_wd(torch.zeros(29, 1000))
