"""The loop-closure part of the C ABI without a GPU: the two records as a C compiler lays them out against botlab_amd._capi, the numpy
dtypes and the sizes include/botlab_hip.h states; the exports; the flags and limits."""
import ctypes
import os
import re
import subprocess

import botlab_amd as bl
from botlab_amd import _capi

import loop_closure_model as lcm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "botlab_hip.h")
FUNCTIONS = ("bl_loopclose_create", "bl_loopclose_destroy", "bl_loopclose_find", "bl_loopclose_candidates", "bl_loopclose_edges",
             "bl_loopclose_submap", "bl_loopclose_last_device_ms")

PROGRAM = r"""
#include <stddef.h>
#include <stdio.h>
#include "botlab_hip.h"
#define P(s, f) printf(#s "." #f " %zu\n", offsetof(s, f))
int main(void)
{
    P(bl_loopclose_params_t, stride); P(bl_loopclose_params_t, min_gap); P(bl_loopclose_params_t, radius); P(bl_loopclose_params_t, w);
    P(bl_loopclose_params_t, submap_cells); P(bl_loopclose_params_t, max_laser); P(bl_loopclose_params_t, hit); P(bl_loopclose_params_t, miss);
    P(bl_loopclose_params_t, match); P(bl_loopclose_params_t, prior);
    printf("bl_loopclose_params_t.sizeof %zu\n", sizeof(bl_loopclose_params_t));
    P(bl_loopclose_candidate_t, q); P(bl_loopclose_candidate_t, j); P(bl_loopclose_candidate_t, first); P(bl_loopclose_candidate_t, count);
    P(bl_loopclose_candidate_t, flags); P(bl_loopclose_candidate_t, pad); P(bl_loopclose_candidate_t, result);
    P(bl_loopclose_candidate_t, moments); P(bl_loopclose_candidate_t, edge);
    printf("bl_loopclose_candidate_t.sizeof %zu\n", sizeof(bl_loopclose_candidate_t));
    printf("flags %d %d %d %d\n", BL_LC_NOT_ACCEPTED, BL_LC_TIED, BL_LC_ON_EDGE, BL_LC_TOO_MANY_RAYS);
    printf("limits %d %d %d %d\n", BL_LC_MAX_CANDIDATES, BL_LC_MAX_W, BL_LC_MIN_SUBMAP, BL_LC_MAX_SUBMAP);
    return 0;
}
"""


def _compiled_layout(tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(PROGRAM)
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = {}
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        key, *vals = line.split()
        out[key] = [int(v) for v in vals]
    return out


def test_records_as_c_lays_them_out(tmp_path):
    c = _compiled_layout(tmp_path)
    for struct, layout, ct, dt in (("bl_loopclose_params_t", lcm.PARAMS_LAYOUT, _capi.LoopCloseParams, None),
                                   ("bl_loopclose_candidate_t", lcm.CANDIDATE_LAYOUT, _capi.LoopCloseCandidate, lcm.CANDIDATE_DTYPE)):
        for field, offset in layout:
            if field is None:
                assert c[struct + ".sizeof"] == [offset] and ctypes.sizeof(ct) == offset
                continue
            assert c[f"{struct}.{field}"] == [offset], (struct, field)
            assert getattr(ct, field).offset == offset, (struct, field)
            if dt is not None:
                assert dt.fields[field][1] == offset
        if dt is not None:
            assert dt.itemsize == layout[-1][1] and bl.LOOPCLOSE_CANDIDATE_DTYPE.itemsize == dt.itemsize
            assert {k: v[1] for k, v in bl.LOOPCLOSE_CANDIDATE_DTYPE.fields.items()} == {k: v[1] for k, v in dt.fields.items()}
    assert c["flags"] == [lcm.NOT_ACCEPTED, lcm.TIED, lcm.ON_EDGE, lcm.TOO_MANY_RAYS] == [bl.LC_NOT_ACCEPTED, bl.LC_TIED, bl.LC_ON_EDGE, bl.LC_TOO_MANY_RAYS]
    assert c["limits"] == [lcm.MAX_CANDIDATES, lcm.MAX_W, lcm.MIN_SUBMAP, lcm.MAX_SUBMAP]


def test_the_header_states_the_sizes():
    text = open(HEADER).read()
    assert re.search(r"\} bl_loopclose_params_t;\s*/\* 84 bytes: offsets 0, 4, 8, 12, 16, 20, 24, 28, 32, 60 \*/", text)
    assert re.search(r"\} bl_loopclose_candidate_t;\s*/\* 272 bytes: offsets 0, 4, 8, 12, 16, 20, 24, 80, 192 \*/", text)
    assert "loop closure  (DESIGN.md 4.33)" in text


def test_exports_and_bindings():
    lib = _capi.load()
    for name in FUNCTIONS:
        assert hasattr(lib, name), name
        assert name in _capi.SIGNATURES
    assert callable(bl.LoopCloser)
    # a null handle is refused, not dereferenced
    n = ctypes.c_int(7)
    assert lib.bl_loopclose_find(None, None, None, None, ctypes.byref(n)) == 2 and n.value == 7
    assert lib.bl_loopclose_edges(None, ctypes.byref(n), None) == 2
    assert lib.bl_loopclose_submap(None, 0, None, None) == 2
    lib.bl_loopclose_destroy(None)
