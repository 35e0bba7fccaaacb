"""The place-recognition part of the C ABI without a GPU: the two records as a C compiler lays them out against botlab_amd._capi, the
numpy dtypes and the sizes include/botlab_hip.h states; the exports; the argument errors that need no device."""
import ctypes
import os
import re
import subprocess

import botlab_amd as bl
from botlab_amd import _capi

import place_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "botlab_hip.h")
FUNCTIONS = ("bl_loopclose_find_places", "bl_loopclose_places", "bl_loopclose_descriptors")
PLACE_FIELDS = ("q", "j", "shift", "key", "overlap", "bits_q", "bits_j", "partner")
PARAM_FIELDS = ("bins_per_meter", "max_range", "dilate", "min_key", "min_bits")

PROGRAM = r"""
#include <stddef.h>
#include <stdio.h>
#include "botlab_hip.h"
#define P(s, f) printf(#s "." #f " %zu\n", offsetof(s, f))
int main(void)
{
    P(bl_place_params_t, bins_per_meter); P(bl_place_params_t, max_range); P(bl_place_params_t, dilate); P(bl_place_params_t, min_key);
    P(bl_place_params_t, min_bits);
    printf("bl_place_params_t.sizeof %zu\n", sizeof(bl_place_params_t));
    P(bl_place_t, q); P(bl_place_t, j); P(bl_place_t, shift); P(bl_place_t, key); P(bl_place_t, overlap); P(bl_place_t, bits_q);
    P(bl_place_t, bits_j); P(bl_place_t, partner);
    printf("bl_place_t.sizeof %zu\n", sizeof(bl_place_t));
    printf("constants %d %d\n", BL_PLACE_SECTORS, BL_PLACE_BINS);
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
    for struct, layout, ct, dts in (("bl_place_params_t", pm.PARAMS_LAYOUT, _capi.PlaceParams, ()),
                                    ("bl_place_t", pm.PLACE_LAYOUT, _capi.Place, (pm.PLACE_DTYPE, bl.LOOPCLOSE_PLACE_DTYPE))):
        for field, offset in layout:
            if field is None:
                assert c[struct + ".sizeof"] == [offset] and ctypes.sizeof(ct) == offset
                assert all(dt.itemsize == offset for dt in dts)
                continue
            assert c[f"{struct}.{field}"] == [offset], (struct, field)
            assert getattr(ct, field).offset == offset, (struct, field)
            assert all(dt.fields[field][1] == offset for dt in dts)
    assert tuple(n for n, _ in pm.PLACE_LAYOUT[:-1]) == PLACE_FIELDS == pm.PLACE_DTYPE.names == bl.LOOPCLOSE_PLACE_DTYPE.names
    assert tuple(n for n, _ in pm.PARAMS_LAYOUT[:-1]) == PARAM_FIELDS == tuple(n for n, _ in _capi.PlaceParams._fields_)
    assert c["constants"] == [pm.SECTORS, pm.BINS] == [_capi.PLACE_SECTORS, _capi.PLACE_BINS] == [64, 32]


def test_the_header_states_the_sizes_and_the_definition():
    text = open(HEADER).read()
    assert re.search(r"\} bl_place_params_t;\s*/\* 20 bytes: offsets 0, 4, 8, 12, 16 \*/", text)
    assert re.search(r"\} bl_place_t;\s*/\* 32 bytes: offsets 0, 4, 8, 12, 16, 20, 24, 28 \*/", text)
    assert "loop closure by place recognition  (DESIGN.md 4.34)" in text
    for word in ("10.185916f", "0.09817477f", "(int)floorf(theta * K) & 63", "min((int)(range * bins_per_meter), 31)", "untuned knobs",
                 "motion during the scan", "s < 32 ? s : s - 64"):
        assert word in text, word


def test_exports_and_bindings():
    lib = _capi.load()
    for name in FUNCTIONS:
        assert hasattr(lib, name), name
        assert name in _capi.SIGNATURES
    assert callable(bl.LoopCloser.find_places) and callable(bl.LoopCloser.places) and callable(bl.LoopCloser.descriptors)


def test_null_pointers_are_refused_not_dereferenced():
    lib = _capi.load()
    n = ctypes.c_int(7)
    prm, pl = _capi.LoopCloseParams(), _capi.PlaceParams()
    assert lib.bl_loopclose_find_places(None, None, None, None, None, ctypes.byref(n)) == 2 and n.value == 7
    assert lib.bl_loopclose_find_places(None, None, None, ctypes.byref(prm), ctypes.byref(pl), ctypes.byref(n)) == 2 and n.value == 7
    assert lib.bl_loopclose_places(None, ctypes.byref(n), None) == 2 and n.value == 7
    assert lib.bl_loopclose_descriptors(None, ctypes.byref(n), None, None) == 2 and n.value == 7
    assert lib.bl_last_error()
