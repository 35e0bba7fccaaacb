"""include/botlab/local_planner.hpp compiles as a C++11 host translation unit (tests/cpp/check_local_planner.cpp, syntax only), and
the structs of the Python binding have the sizes the header states."""
import ctypes
import os
import subprocess

from botlab_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_compiles():
    subprocess.check_call(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "check_local_planner.cpp")])


def test_struct_sizes():
    assert ctypes.sizeof(_capi.LocalPlanState) == 32 and _capi.LocalPlanState.v.offset == 24
    assert ctypes.sizeof(_capi.LocalPlanParams) == 56 and _capi.LocalPlanParams.n_v.offset == 28
    assert ctypes.sizeof(_capi.LocalPlanResult) == 32 and _capi.LocalPlanResult.cost.offset == 16
