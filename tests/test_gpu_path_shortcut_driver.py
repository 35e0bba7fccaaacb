"""MotionPlannerT::planPathShortcut (include/botlab/planning_dropin.hpp) through the C++ program (tests/cpp/path_shortcut_test.cpp)
on the obstacle map, against the model's field path (tests/nav_field_model.py) shortened by the model (tests/path_shortcut_model.py).
This is the one path shortcutting test that runs the navigation field on the device; it sits in a file of its own."""
import numpy as np
import pytest

import helpers
import path_shortcut_model as psm
import test_path_shortcut_model_cpu as cpu
from test_gpu_path_shortcut_cpp import build, run, same

pytestmark = pytest.mark.gpu
CPM = helpers.CPM_DEFAULT


def test_plan_path_shortcut_equals_model_field_path_and_model_shortcut(maps, tmp_path):
    world, poses = cpu.map_case(maps)                                # the model's planPathOptimal from the same start to the same goal
    p = psm.Params(0.2, 32, 2048)
    exp, _, _ = psm.shortcut_poses(world.ok(0.2), poses, world.origin, CPM, p)
    gx = float(world.origin[0]) + (124 + 0.5) * float(world.mpc)
    gy = float(world.origin[1]) + (126 + 0.5) * float(world.mpc)
    plan = (int(poses["utime"][0]), float(poses["x"][0]), float(poses["y"][0]), float(poses["theta"][0]), gx, gy)
    r = run(build(str(tmp_path)), str(tmp_path), world, poses, p, plan)
    print("planPathShortcut:", len(poses), "->", len(r["D"]), "poses")
    assert same(r["D"], exp) and 2 <= len(exp) < len(poses)
    assert same(r["S"][0], exp)
