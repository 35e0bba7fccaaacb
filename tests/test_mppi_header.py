"""MppiPlannerT compiles as a C++11 host translation unit (tests/cpp/check_mppi_planner.cpp, syntax only, with the structs' sizes and
offsets asserted), and the structs and constants of the Python binding and of the model are the header's."""
import ctypes
import os
import re
import subprocess

from botlab_amd import _capi, host
import mppi_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_compiles():
    subprocess.check_call(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "check_mppi_planner.cpp")])


def test_struct_layouts_and_constants():
    offs = lambda s: [getattr(s, n).offset for n, _ in s._fields_]
    assert ctypes.sizeof(_capi.MppiParams) == 72 and offs(_capi.MppiParams) == [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 52, 56, 60, 64]
    assert ctypes.sizeof(_capi.MppiState) == 40 and offs(_capi.MppiState) == [0, 32, 36]
    assert ctypes.sizeof(_capi.MppiResult) == 56 and offs(_capi.MppiResult) == [0, 4, 8, 12, 16, 24, 32, 40, 48, 52]
    assert [host.MPPI_RESULT_DTYPE.fields[n][1] for n in host.MPPI_RESULT_DTYPE.names] == offs(_capi.MppiResult)
    assert host.MPPI_RESULT_DTYPE == mm.RESULT and host.MPPI_FELL_BACK == mm.FELL_BACK
    text = open(os.path.join(ROOT, "include", "botlab_hip.h")).read()
    assert "} bl_mppi_params_t;                    /* 72 bytes: offsets 0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 52, 56, 60, 64 */" in text
    assert "} bl_mppi_state_t;                     /* 40 bytes: offsets 0, 32, 36 */" in text
    assert "} bl_mppi_result_t;                    /* 56 bytes: offsets 0, 4, 8, 12, 16, 24, 32, 40, 48, 52 */" in text
    for name, value in (("MAX_SAMPLES", mm.MAX_SAMPLES), ("MAX_HORIZON", mm.MAX_HORIZON), ("MAX_SUB", mm.MAX_SUB), ("MAX_STEPS", mm.MAX_STEPS),
                        ("FELL_BACK", mm.FELL_BACK)):
        assert "#define BL_MPPI_%s %d\n" % (name, value) in text, name
    assert "#define BL_MPPI_MAX_LAMBDA (1 << 30)" in text and "#define BL_MPPI_MAX_Q (1 << 21)" in text
    assert mm.MAX_LAMBDA == 1 << 30 and mm.MAX_Q == 1 << 21
    assert re.search(r"table\[i\] = \(table\[i-1\] \* %d\) >> 32" % mm.TABLE_MUL, text)


def test_weight_table_of_the_library_is_the_models():
    out = (ctypes.c_uint32 * 257)()
    _capi.load().bl_mppi_weight_table(out)                       # host arithmetic: no GPU
    assert list(out) == mm.weight_table()
