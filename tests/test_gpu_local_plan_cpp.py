"""LocalPlannerT (include/botlab/local_planner.hpp; tests/cpp/local_planner_test.cpp built with g++ -std=c++11) on the obstacle map:
three commands and the winning rollout of the first against the model (tests/local_plan_model.py)."""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import local_plan_model as lpm
import test_local_plan_model_cpu as cpu
from test_gpu_nav_field_driver import _write_map_file

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def test_cpp_class_matches_the_model():
    world, _, _ = cpu.loop_world()
    p = lpm.Params(**cpu.LOOP_PARAMS)
    start = cpu.loop_start(world)
    gx, gy = cpu.cell_centre(world, *cpu.LOOP_GOAL)
    states = [(1001, start, F32(0.0), F32(0.0)),                                              # at rest, facing the wall
              (1002, cpu.cell_centre(world, 98, 134) + (F32(-1.4),), F32(0.3), F32(-0.2)),    # in the passage, moving
              (1003, (gx, gy, F32(0.5)), F32(0.1), F32(0.0))]                                 # on the goal: REACHED
    blob = struct.pack("<7f7i", *[float(f) for f in p.floats()], p.n_v, p.n_w, p.n_steps, p.w_field, p.w_heading, p.w_clear, p.w_speed)
    for utime, pose, v, w in states:
        blob += struct.pack("<q5f", utime, *[float(f) for f in pose], float(v), float(w))
    with tempfile.TemporaryDirectory() as td:
        exe, run, outp, mapfile = (os.path.join(td, n) for n in ("local_planner_test", "run.bin", "out.bin", "m.map"))
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "local_planner_test.cpp"),
                               "-L" + os.path.join(ROOT, "botlab_amd"), "-lbotlab_hip", "-Wl,-rpath," + os.path.join(ROOT, "botlab_amd"), "-o", exe])
        open(run, "wb").write(blob)
        _write_map_file(mapfile, world.cells, world.origin, world.mpc)
        r = subprocess.run([exe, mapfile, run, outp, str(cpu.LOOP_GOAL[0]), str(cpu.LOOP_GOAL[1]), str(cpu.LOOP_REACH)], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0 and b"local_planner_test ok: 3 commands" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
        raw = open(outp, "rb").read()
    off, flags = 0, []
    for k, (utime, pose, v, w) in enumerate(states):
        exp, _ = lpm.command(world, p, pose, v, w)
        assert raw[off:off + 32] == struct.pack("<q", utime) + exp["trans_v"].tobytes() + exp["angular_v"].tobytes() + exp["flags"].tobytes() + \
            exp["index"].tobytes() + exp["cost"].tobytes(), (k, exp)
        flags.append(int(exp["flags"]))
        if k == 0:
            first = exp
        off += 32
    assert flags == [0, 0, lpm.REACHED]
    vt, wt = lpm.tables(p, states[0][2], states[0][3])
    c = int(first["index"])
    arc = lpm.rollout(states[0][1], vt[c % p.n_v], wt[c // p.n_v], p)
    assert raw[off:] == b"".join(F32(q[0]).tobytes() + F32(q[1]).tobytes() + F32(q[2]).tobytes() for q in arc)
