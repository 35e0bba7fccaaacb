"""include/botlab/likelihood_field.hpp and the OccupancyGridSLAMT switch built on it compile as a C++11 host translation unit
(tests/cpp/check_likelihood_field.cpp, syntax only), and the parameter struct of the Python binding has the header's layout."""
import ctypes
import os
import subprocess

from botlab_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_compiles():
    subprocess.check_call(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "check_likelihood_field.cpp")])


def test_struct_layout():
    p = _capi.LFieldParams
    assert ctypes.sizeof(p) == 16 and (p.sigma.offset, p.max_cells.offset, p.occ_min.offset, p.peak.offset) == (0, 4, 8, 12)
