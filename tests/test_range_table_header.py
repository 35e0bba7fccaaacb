"""include/botlab/range_table.hpp, the table forms of BeamModelT and ParticleFilterT and OccupancyGridSLAMT::setBeamRangeTable compile as
a C++11 host translation unit (tests/cpp/check_range_table.cpp, syntax only, with the struct's size asserted), the Python binding has
the header's layout, the library exports every symbol the range table's section declares, and the refusals that need no GPU."""
import ctypes
import os
import re
import subprocess

from botlab_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE_SYMBOLS = ["bl_rangetable_build", "bl_rangetable_create", "bl_rangetable_debug_lookup", "bl_rangetable_destroy", "bl_rangetable_directions",
                 "bl_rangetable_info", "bl_rangetable_last_device_ms", "bl_rangetable_read", "bl_rangetable_reweigh_pf", "bl_rangetable_scores",
                 "bl_rangetable_update"]


def _declared(path, prefix):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", path)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(%s[a-z0-9_]+)\s*\(" % prefix, text)))


def test_header_compiles():
    subprocess.check_call(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "check_range_table.cpp")])
    # the C header alone, as C
    subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"],
                   input=b'#include "botlab_hip.h"\nint main(void) { return (int)sizeof(bl_rangetable_info_t) - 32; }\n', check=True)


def test_struct_layout():
    p = _capi.RangeTableInfo
    assert ctypes.sizeof(p) == 32
    assert tuple(getattr(p, f).offset for f, _ in p._fields_) == (0, 4, 8, 12, 16, 20, 24)
    text = open(os.path.join(ROOT, "include", "botlab_hip.h")).read()
    assert "32 bytes: offsets 0, 4, 8, 12, 16, 20, 24" in text and "#define BL_RANGETABLE_NONE 0xFFFF" in text


def test_library_exports_the_range_table_symbols():
    assert _declared("botlab_hip.h", "bl_rangetable_") == TABLE_SYMBOLS
    lib = _capi.load()
    for n in TABLE_SYMBOLS:
        assert hasattr(lib, n) and n in _capi.SIGNATURES, n


def test_refusals_without_a_gpu():
    """Null handles and null outputs are refused before anything touches a device."""
    lib = _capi.load()
    h = ctypes.c_void_p()
    assert lib.bl_rangetable_create(None, 256, ctypes.byref(h)) == 2 and not h.value
    info = _capi.RangeTableInfo()
    ms = ctypes.c_float()
    assert lib.bl_rangetable_info(None, ctypes.byref(info)) == 2
    assert lib.bl_rangetable_build(None, None, None) == 2
    assert lib.bl_rangetable_update(None, None, 0, 0, 1, 1) == 2
    assert lib.bl_rangetable_read(None, 0, 0, 1, 1, None) == 2
    assert lib.bl_rangetable_directions(None, None) == 2
    assert lib.bl_rangetable_last_device_ms(None, ctypes.byref(ms)) == 2
    assert lib.bl_rangetable_scores(None, None, None, None, 0, None) == 2
    assert lib.bl_rangetable_reweigh_pf(None, None, None, None, None) == 2
    assert lib.bl_rangetable_debug_lookup(None, None, None, None, None, None, None, None) == 2
    lib.bl_rangetable_destroy(None)
