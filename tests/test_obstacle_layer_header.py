"""include/botlab/obstacle_layer.hpp and MotionPlannerT::setMapWithObstacles compile as a C++11 host translation unit
(tests/cpp/check_obstacle_layer.cpp, syntax only, with the struct sizes asserted), and the structs of the Python binding have the
header's layout."""
import ctypes
import os
import subprocess

from botlab_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_compiles():
    subprocess.check_call(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "check_obstacle_layer.cpp")])


def test_struct_layouts():
    p = _capi.ObsLayerParams
    assert ctypes.sizeof(p) == 20
    assert (p.max_range.offset, p.occ_min.offset, p.tol_cells.offset, p.ttl_scans.offset, p.min_hits.offset) == (0, 4, 8, 12, 16)
    s = _capi.ObsLayerStats
    assert ctypes.sizeof(s) == 40
    assert (s.n.offset, s.valid_rays.offset, s.rays_by_class.offset, s.hit_cells.offset, s.cleared_cells.offset, s.live_cells.offset) == (0, 4, 8, 28, 32, 36)
    assert s.rays_by_class.size == 20


def test_header_states_the_layout_the_binding_has():
    text = open(os.path.join(ROOT, "include", "botlab_hip.h")).read()
    assert "20 bytes: offsets 0, 4, 8, 12, 16" in text and "40 bytes: offsets 0, 4, 8, 28, 32, 36" in text
    for name in ("bl_obslayer_create", "bl_obslayer_update", "bl_obslayer_compose", "bl_obslayer_upload", "bl_obslayer_last_device_ms"):
        assert name in _capi.SIGNATURES
