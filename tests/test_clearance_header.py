"""include/botlab/clearance_grid.hpp and the leap forms of BeamModelT and ParticleFilterT compile as a C++11 host translation unit
(tests/cpp/check_clearance_grid.cpp, syntax only, with the struct's size asserted), the Python binding has the header's layout, the
library exports every symbol the clearance grid's section declares, and the refusals that need no GPU."""
import ctypes
import os
import re
import subprocess

import botlab_amd as bl
from botlab_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLEARANCE_SYMBOLS = ["bl_clearance_build", "bl_clearance_create", "bl_clearance_debug_cast", "bl_clearance_destroy", "bl_clearance_info",
                     "bl_clearance_last_device_ms", "bl_clearance_read", "bl_clearance_reweigh_pf", "bl_clearance_scores", "bl_clearance_update"]


def _declared(path, prefix):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", path)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(%s[a-z0-9_]+)\s*\(" % prefix, text)))


def test_header_compiles():
    subprocess.check_call(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "check_clearance_grid.cpp")])
    # the C header alone, as C
    subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"],
                   input=b'#include "botlab_hip.h"\nint main(void) { return (int)sizeof(bl_clearance_info_t) - 32; }\n', check=True)


def test_struct_layout():
    p = _capi.ClearanceInfo
    assert ctypes.sizeof(p) == 32
    assert [f for f, _ in p._fields_] == ["width", "height", "cap", "occ_min", "built", "pad", "bytes"]
    assert tuple(getattr(p, f).offset for f, _ in p._fields_) == (0, 4, 8, 12, 16, 20, 24)
    text = open(os.path.join(ROOT, "include", "botlab_hip.h")).read()
    assert "} bl_clearance_info_t;                 /* 32 bytes: offsets 0, 4, 8, 12, 16, 20, 24 */" in text


def test_library_exports_the_clearance_symbols():
    assert _declared("botlab_hip.h", "bl_clearance_") == CLEARANCE_SYMBOLS
    lib = _capi.load()
    for n in CLEARANCE_SYMBOLS:
        assert hasattr(lib, n) and n in _capi.SIGNATURES, n
    for n in ("ClearanceGrid",):
        assert n in bl.__all__ and hasattr(bl, n)
    for cls, names in ((bl.ClearanceGrid, ("build", "update", "read", "info", "lastDeviceMs")),
                       (bl.BeamModel, ("scores_leap", "reweigh_leap", "debug_leap")), (bl.ParticleFilter, ("reweigh_beam_leap",))):
        assert all(callable(getattr(cls, n)) for n in names)


def test_refusals_without_a_gpu():
    """Null handles and null outputs are refused before anything touches a device."""
    lib = _capi.load()
    h = ctypes.c_void_p()
    assert lib.bl_clearance_create(None, 64, ctypes.byref(h)) == 2 and not h.value
    info = _capi.ClearanceInfo()
    ms = ctypes.c_float()
    assert lib.bl_clearance_info(None, ctypes.byref(info)) == 2
    assert lib.bl_clearance_build(None, None, 1) == 2
    assert lib.bl_clearance_update(None, None, 0, 0, 1, 1) == 2
    assert lib.bl_clearance_read(None, 0, 0, 1, 1, None) == 2
    assert lib.bl_clearance_last_device_ms(None, ctypes.byref(ms)) == 2
    assert lib.bl_clearance_scores(None, None, None, None, 0, None) == 2
    assert lib.bl_clearance_reweigh_pf(None, None, None, None, None) == 2
    assert lib.bl_clearance_debug_cast(None, None, None, None, None, None, None, None, None, None) == 2
    lib.bl_clearance_destroy(None)
