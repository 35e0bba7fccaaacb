"""ObstacleTrackerT (include/botlab/obstacle_tracks.hpp) and MotionPlannerT::setMapWithTracks (include/botlab/planning_dropin.hpp),
built with g++ -std=c++11 from tests/cpp/obstacle_tracks_test.cpp and run over the life-cycle and the compose script: everything the
binary writes equals the model's recorded values, the host reference walked beside the device inside the binary agrees at every
update, and the planner's distances equal the Python host's transform of the model's composed grid."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import botlab_amd as bl
import obstacle_tracks_stream as stream
import test_obstacle_tracks_model_cpu as cpu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program():
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "obstacle_tracks_test")
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "obstacle_tracks_test.cpp"), "-L" + os.path.join(ROOT, "botlab_amd"),
                               "-lbotlab_hip", "-Wl,-rpath," + os.path.join(ROOT, "botlab_amd"), "-o", exe])
        yield exe, td


@pytest.mark.parametrize("name,w,h", [("lifecycle", 37, 23), ("compose", 131, 67)])
def test_cpp_tracker_and_planner_equal_the_model(gpu_ctx, program, name, w, h):
    exe, td = program
    script, model, _ = cpu.model_of(name, w, h)
    data, sent = stream.encode(script, model, refused_compose=False)      # a refused compose ends a C++ program: check() aborts
    inp, outp = os.path.join(td, name + ".in"), os.path.join(td, name + ".out")
    with open(inp, "wb") as f:
        f.write(data)
    r = subprocess.run([exe, inp, outp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0 and b"obstacle_tracks_test ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    composes = stream.check(open(outp, "rb").read(), script, model, sent, distances=True)
    assert len(composes) >= 1
    k, composed, dist = composes[-1]
    g = bl.OccupancyGrid.from_cells(composed, script.origin, script.mpc, ctx=gpu_ctx)
    d = bl.ObstacleDistanceGrid(ctx=gpu_ctx)
    try:
        d.setDistances(g)
        assert np.array_equal(d.cells().view(np.uint32), dist.view(np.uint32))
    finally:
        d.close()
        g.close()
