"""LocalPlannerT::commandMoving, ObstacleTrackerT::composeStatic and MotionPlannerT::setMapWithStaticObstacles compile as a C++11 host
translation unit (tests/cpp/check_local_plan_moving.cpp, syntax only, with the struct's size and offsets asserted), and the struct
and the constants of the Python binding and of the model are the header's."""
import ctypes
import os
import re
import subprocess

from botlab_amd import _capi
import local_plan_moving_model as lmm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_compiles():
    subprocess.check_call(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "check_local_plan_moving.cpp")])


def test_struct_layout_and_constants():
    s = _capi.LocalPlanMoving
    assert ctypes.sizeof(s) == 16
    assert [(n, getattr(s, n).offset) for n, _ in s._fields_] == [("steps_per_update", 0), ("margin_cells", 4), ("lead_steps", 8), ("reserved", 12)]
    text = open(os.path.join(ROOT, "include", "botlab_hip.h")).read()
    assert "} bl_localplan_moving_t;               /* 16 bytes: offsets 0, 4, 8, 12 */" in text
    m = re.search(r"#define BL_LOCALPLAN_MOVING_BYTES \((\d+) \* 1024\)", text)
    assert m and int(m.group(1)) * 1024 == lmm.MOVING_BYTES
    assert "#define BL_LOCALPLAN_MAX_MARGIN %d\n" % lmm.MAX_MARGIN in text
    for name in ("bl_localplan_commands_moving", "bl_localplan_debug_costs_moving", "bl_localplan_debug_moving_path", "bl_obstracks_compose_static"):
        assert name in _capi.SIGNATURES
