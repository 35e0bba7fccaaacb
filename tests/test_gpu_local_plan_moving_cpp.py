"""LocalPlannerT::commandMoving / commandsMoving, ObstacleTrackerT::composeStatic and MotionPlannerT::setMapWithStaticObstacles
(tests/cpp/local_plan_moving_test.cpp built with g++ -std=c++11) on a 64 x 64 room with a blob that moves and one that stands: the
two composed grids and the commands equal numbers the Python model wrote to a file."""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import local_plan_cases as lc
import local_plan_model as lpm
import local_plan_moving_cases as mc
import local_plan_moving_model as lmm
import obstacle_tracks_model as tm
import test_local_plan_model_cpu as cpu
from test_gpu_nav_field_driver import _write_map_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
W = H = 64
GOAL, REACH = (40, 40), 1
UPDATES = 6
LAYER = dict(max_range=5.0, occ_min=1, tol_cells=1, ttl_scans=3, min_hits=1)
TRACKS = dict(tm.BASE, max_cells=9)
PARAMS = dict(v_min=0.0, v_max=0.5, w_max=2.0, acc_v=10.0, acc_w=30.0, dt_control=0.1, dt_sim=0.05, n_v=3, n_w=9, n_steps=20, w_field=3, w_heading=1,
              w_clear=1, w_speed=2)
MOVING = (2, 1, 0)
ATS = [(16.4, 14.3, -1.5), (13.5, 15.5, -1.2), (30.5, 30.5, 0.0), (40.5, 40.5, 1.0), (-5.0, 3.0, 0.0)]


def scene():
    """(cells, the model's tracker after UPDATES updates, the live cells per update, the model's static composition, its world)."""
    cells = cpu.uniform_cells(W, H)
    live_at = mc.blob_scene(W, H)
    t = tm.Tracker(W, H, **TRACKS)
    lives = [live_at(n) for n in range(1, UPDATES + 1)]
    for n, live in enumerate(lives, 1):
        t.update(live, n)
    composed = lmm.compose_static(t, lives[-1], UPDATES, cells)
    world = cpu.make_world(composed, cpu.ORIGIN, cpu.MPC, [GOAL], REACH)[0]
    return cells, t, lives, composed, world


def expected():
    cells, t, lives, composed, world = scene()
    p, m = lpm.Params(**PARAMS), lmm.Moving(*MOVING)
    states = [(1000 + k, lc.on_cell(world, *a), F32(0.2), F32(0.0)) for k, a in enumerate(ATS)]
    recs = [lmm.command_moving(world, p, t.slots, m, pose, v, w) for _, pose, v, w in states]
    return cells, t, lives, composed, world, p, m, states, recs


def test_the_scene_is_what_it_is_meant_to_be():
    cells, t, lives, composed, world, p, m, states, recs = expected()
    assert len(lmm.used_slots(t.slots)) == 1 and len(t.tracks()) == 2
    plain = np.where(lives[-1], 127, cells)
    assert np.count_nonzero(composed != plain) == 9 and np.count_nonzero(composed == 127) == 9      # the moving blob out, the standing one in
    flags = [int(r[0]["flags"]) for r in recs]
    assert flags == [0, 0, 0, lpm.REACHED, lpm.OFF_FIELD], flags
    refused = [int(np.count_nonzero(r[2])) for r in recs[:2]]
    assert all(refused), refused
    plain_rec = lpm.command(world, p, *states[0][1:])[0]
    assert plain_rec.tobytes() != recs[0][0].tobytes()              # the moving rule changes the first command
    print("refused candidates", refused, "indices", [int(r[0]["index"]) for r in recs])


@pytest.mark.gpu
def test_cpp_classes_match_the_model():
    cells, t, lives, composed, world, p, m, states, recs = expected()
    blob = struct.pack("<7f7i", *[float(f) for f in p.floats()], p.n_v, p.n_w, p.n_steps, p.w_field, p.w_heading, p.w_clear, p.w_speed)
    blob += struct.pack("<4i", m.q, m.margin, m.lead, 0)
    blob += struct.pack("<f4i", LAYER["max_range"], LAYER["occ_min"], LAYER["tol_cells"], LAYER["ttl_scans"], LAYER["min_hits"])
    blob += struct.pack("<8i", *[TRACKS[k] for k in tm.PARAM_NAMES])
    blob += struct.pack("<i", UPDATES)
    for n, live in enumerate(lives, 1):
        blob += live.astype(np.uint8).tobytes() + np.where(live, n, 0).astype("<u4").tobytes() + struct.pack("<I", n)
    blob += struct.pack("<i", len(states))
    for utime, pose, v, w in states:
        blob += struct.pack("<q5f", utime, *[float(f) for f in pose], float(v), float(w))
    with tempfile.TemporaryDirectory() as td:
        exe, run, outp, mapfile = (os.path.join(td, n) for n in ("local_plan_moving_test", "run.bin", "out.bin", "m.map"))
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "local_plan_moving_test.cpp"),
                               "-L" + os.path.join(ROOT, "botlab_amd"), "-lbotlab_hip", "-Wl,-rpath," + os.path.join(ROOT, "botlab_amd"), "-o", exe])
        open(run, "wb").write(blob)
        _write_map_file(mapfile, cells, cpu.ORIGIN, cpu.MPC)
        r = subprocess.run([exe, mapfile, run, outp, str(GOAL[0]), str(GOAL[1]), str(REACH)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0 and b"local_plan_moving_test ok: 6 updates, 5 commands" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
        raw = open(outp, "rb").read()
    n = W * H
    assert raw[:n] == composed.tobytes() and raw[n:2 * n] == composed.tobytes()
    off = 2 * n
    for k, ((utime, pose, v, w), (exp, _, _)) in enumerate(zip(states, recs)):
        assert raw[off:off + 32] == struct.pack("<q", utime) + exp["trans_v"].tobytes() + exp["angular_v"].tobytes() + exp["flags"].tobytes() + \
            exp["index"].tobytes() + exp["cost"].tobytes(), (k, exp)
        off += 32
    assert off == len(raw)
