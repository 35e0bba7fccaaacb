"""ObstacleDistanceGrid::euclidean and MotionPlannerT::setMetricClearance (include/botlab/botlab_dropin.hpp, planning_dropin.hpp;
tests/cpp/metric_clearance_test.cpp built with g++ -std=c++11) on the diagonal-gap maps.  The expected values come from the fixture
tests/golden/metric_clearance_gap.txt, which is what the Python models give (checked here first)."""
import importlib.util
import os
import subprocess

import pytest

import helpers
import test_edt_model_cpu as cpu
from test_gpu_nav_field_driver import _write_map_file

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(helpers.GOLDEN, "metric_clearance_gap.txt")


def _maker():
    spec = importlib.util.spec_from_file_location("make_metric_clearance_fixture", os.path.join(helpers.GOLDEN, "make_metric_clearance_fixture.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build(td):
    exe = os.path.join(td, "metric_clearance_test")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "metric_clearance_test.cpp"), "-L" + os.path.join(ROOT, "botlab_amd"), "-lbotlab_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "botlab_amd"), "-o", exe])
    return exe


def test_cpp_metric_clearance(tmp_path):
    mk = _maker()
    assert open(FIXTURE).read() == mk.text()                         # the fixture is the models' answer
    td = str(tmp_path)
    files = []
    for offset in (5, 7):
        files.append(os.path.join(td, "gap%d.map" % offset))
        _write_map_file(files[-1], cpu.gap_cells(offset), mk.ORIGIN, mk.MPC)
    sx, sy = mk.centre(cpu.GAP_START)
    gx, gy = mk.centre(cpu.GAP_GOAL)
    r = subprocess.run([build(td)] + files + [FIXTURE] + [repr(float(v)) for v in (sx, sy, gx, gy)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=300)
    assert r.returncode == 0 and b"metric_clearance_test ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
