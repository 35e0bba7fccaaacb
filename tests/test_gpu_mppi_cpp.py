"""MppiPlannerT (include/botlab/mppi_planner.hpp; tests/cpp/mppi_planner_test.cpp built with g++ -std=c++11) on the obstacle map: three
consecutive commands through command() / commandMoving() and advance(), and the sequence held after them, against the model
(tests/mppi_model.py) as bytes."""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import mppi_cases as mc
import mppi_model as mm
import test_local_plan_model_cpu as cpu
from test_gpu_nav_field_driver import _write_map_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
PARAMS = dict(mc.LOOP, n_samples=300, seed=0xABCDEF0123)


def expected():
    """Three ticks of the model's loop from the loop world's start: (utime, pose, v, w) per tick, the records, the last sequence."""
    world = cpu.loop_world()[0]
    p = mm.Params(**PARAMS)
    pose, v, w = cpu.loop_start(world), F32(0), F32(0)
    seq = np.zeros((p.T, 2), np.int32)
    states, recs = [], []
    for tick in range(3):
        states.append((2000 + tick, pose, v, w))
        r, so, _ = mm.plan(world, p, pose, v, w, tick, 0, seq)
        recs.append(r)
        assert int(r["flags"]) in (0, mm.FELL_BACK)
        v, w = F32(r["trans_v"]), F32(r["angular_v"])
        pose = mm.drive(pose, so[0], p)[-1]
        held, seq = so, mm.advance(so, int(r["flags"]))
    return world, p, states, recs, held


def test_the_three_ticks_move_the_robot():
    world, p, states, recs, held = expected()
    assert any(float(r["angular_v"]) != 0.0 for r in recs) and held.any() and len({s[1] for s in states}) == 3


@pytest.mark.gpu
def test_cpp_class_matches_the_model():
    world, p, states, recs, held = expected()
    blob = struct.pack("<8f8iQ", *[float(f) for f in p.floats()], p.K, p.T, p.n_sub, p.lam, p.w_field, p.w_heading, p.w_clear, 0, p.seed)
    assert len(blob) == 72
    for utime, pose, v, w in states:
        blob += struct.pack("<q5f", utime, *[float(f) for f in pose], float(v), float(w))
    with tempfile.TemporaryDirectory() as td:
        exe, run, outp, mapfile = (os.path.join(td, n) for n in ("mppi_planner_test", "run.bin", "out.bin", "m.map"))
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "mppi_planner_test.cpp"),
                               "-L" + os.path.join(ROOT, "botlab_amd"), "-lbotlab_hip", "-Wl,-rpath," + os.path.join(ROOT, "botlab_amd"), "-o", exe])
        open(run, "wb").write(blob)
        _write_map_file(mapfile, world.cells, world.origin, world.mpc)
        r = subprocess.run([exe, mapfile, run, outp, str(cpu.LOOP_GOAL[0]), str(cpu.LOOP_GOAL[1]), str(cpu.LOOP_REACH)], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0 and b"mppi_planner_test ok: 3 commands, 10 controls, 20 rollout poses" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
        raw = open(outp, "rb").read()
    off = 0
    for k, ((utime, pose, v, w), exp) in enumerate(zip(states, recs)):
        assert raw[off:off + 32] == struct.pack("<q", utime) + exp["trans_v"].tobytes() + exp["angular_v"].tobytes() + exp["flags"].tobytes() + \
            exp["index_best"].tobytes() + exp["cost_out"].tobytes(), (k, exp)
        off += 32
    assert raw[off:] == held.astype("<i4").tobytes()
