"""The obstacle tracks in plain C++ on the host (tests/cpp/obstacle_tracks_ref.hpp, the walk that tests/cpp/obstacle_tracks_test.cpp
holds the device against) equal the model: tests/cpp/obstacle_tracks_ref_main.cpp is built with g++ alone and run over the life-cycle,
association, compose and caps scripts.  No GPU and no library."""
import os
import subprocess
import tempfile

import pytest

import obstacle_tracks_stream as stream
import test_obstacle_tracks_model_cpu as cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ref_program():
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "obstacle_tracks_ref_main")
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "obstacle_tracks_ref_main.cpp"), "-o", exe])
        yield exe, td


@pytest.mark.parametrize("name,w,h", [("lifecycle", 37, 23), ("assoc", 37, 23), ("compose", 64, 64), ("shapes", 131, 67), ("caps", 131, 67)])
def test_host_reference_equals_the_model(ref_program, name, w, h):
    exe, td = ref_program
    script, model, _ = cpu.model_of(name, w, h)
    data, sent = stream.encode(script, model)
    assert len(sent) == len(script.steps)
    inp, outp = os.path.join(td, name + ".in"), os.path.join(td, name + ".out")
    with open(inp, "wb") as f:
        f.write(data)
    r = subprocess.run([exe, inp, outp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0 and b"obstacle_tracks_ref_main ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    composes = stream.check(open(outp, "rb").read(), script, model, sent)
    assert name != "compose" or len(composes) == 9
