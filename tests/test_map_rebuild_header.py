"""include/botlab/map_rebuild.hpp and OccupancyGridSLAMT::setScanHistory / rebuildMap compile as a C++11 host translation unit
(tests/cpp/check_map_rebuild.cpp, syntax only, with the struct's size asserted), the Python binding has the header's layout, the library
exports every bl_scanlog_* symbol the header declares, and the argument errors that need no GPU are BL_ERR_ARG."""
import ctypes
import os
import re
import subprocess

from botlab_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCANLOG_SYMBOLS = ["bl_scanlog_append", "bl_scanlog_append_dev_pose", "bl_scanlog_create", "bl_scanlog_destroy", "bl_scanlog_get_poses",
                   "bl_scanlog_get_scan", "bl_scanlog_last_stats", "bl_scanlog_rebuild", "bl_scanlog_set_poses", "bl_scanlog_size"]
BL_ERR_ARG = 2


def test_header_compiles():
    subprocess.check_call(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "check_map_rebuild.cpp")])


def test_struct_layout():
    s = _capi.ScanLogStats
    assert ctypes.sizeof(s) == 64
    got = tuple(getattr(s, f).offset for f, _ in s._fields_)
    assert got == (0, 8, 16, 24, 32, 36, 40, 44, 48, 52, 56, 60)


def test_library_exports_the_scanlog_symbols():
    text = open(os.path.join(ROOT, "include", "botlab_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(bl_scanlog_[a-z0-9_]+)\s*\(", text)))
    assert declared == SCANLOG_SYMBOLS
    lib = _capi.load()
    for n in SCANLOG_SYMBOLS:
        assert hasattr(lib, n) and n in _capi.SIGNATURES, n


def test_argument_errors_that_need_no_gpu():
    lib = _capi.load()
    h = ctypes.c_void_p()
    # refused before anything touches a device (the ctx is not even looked at): a capacity below 1, rays outside 1 .. 8192, over 1 GiB
    for cap, rays in [(0, 290), (-3, 290), (8, 0), (8, 8193), (8193, 8192), (1 << 24, 290)]:
        assert lib.bl_scanlog_create(None, cap, rays, ctypes.byref(h)) == BL_ERR_ARG and not h.value, (cap, rays)
        assert b"bad argument" in lib.bl_last_error()
    assert lib.bl_scanlog_create(None, 8, 290, None) == BL_ERR_ARG
    assert lib.bl_scanlog_create(None, 8, 290, ctypes.byref(h)) == BL_ERR_ARG and not h.value          # no ctx
    # a null log
    pose = _capi.Pose(0, 0.0, 0.0, 0.0)
    scan = _capi.Lidar(0, 0, None, None, None, None)
    stats = _capi.ScanLogStats()
    assert lib.bl_scanlog_size(None) == 0
    assert lib.bl_scanlog_append(None, ctypes.byref(scan), ctypes.byref(pose)) == BL_ERR_ARG
    assert lib.bl_scanlog_append(None, ctypes.byref(scan), None) == BL_ERR_ARG
    assert lib.bl_scanlog_append_dev_pose(None, ctypes.byref(scan), None, 0) == BL_ERR_ARG
    assert lib.bl_scanlog_get_poses(None, 0, 1, ctypes.byref(pose)) == BL_ERR_ARG
    assert lib.bl_scanlog_set_poses(None, 0, 1, ctypes.byref(pose)) == BL_ERR_ARG
    assert lib.bl_scanlog_get_scan(None, 0, None, None, None, None) == BL_ERR_ARG
    assert lib.bl_scanlog_rebuild(None, 0, 1, None, None, 5.0, 3, 1, None, None) == BL_ERR_ARG
    assert lib.bl_scanlog_last_stats(None, ctypes.byref(stats)) == BL_ERR_ARG
    lib.bl_scanlog_destroy(None)
