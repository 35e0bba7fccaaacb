"""BeamModelT (include/botlab/beam_model.hpp), ParticleFilterT::reweighBeam and OccupancyGridSLAMT::setBeamModel, built with
g++ -std=c++11 from tests/cpp/beam_model_test.cpp and tests/cpp/beam_driver_test.cpp:

  * scores, units, debugCast, tables and reweighBeam equal the Python path byte for byte, and both equal the model;
  * the two-wall case from a cloud split between A and B: after reweighBeam the heaviest cluster stands at A.  (The driver seeds its own
    cloud -- at a pose or uniformly -- so a hand-split cloud goes through the filter class, not through the driver.)
  * the driver with the switch never touched and with setBeamModel(false, ...) writes the same bytes; with it on the model is active,
    the control flow is the same and the estimate still tracks the truth."""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import botlab_amd as bl
import beam_cases as bc
import beam_model as bm
import test_gpu_slam_driver as drv
from test_gpu_beam import KEYS, grid_of, scan_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(td, name):
    exe = os.path.join(td, name)
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", name + ".cpp"),
                           "-L" + os.path.join(ROOT, "botlab_amd"), "-lbotlab_hip", "-Wl,-rpath," + os.path.join(ROOT, "botlab_amd"), "-o", exe])
    return exe


def _split_cloud(c, n):
    """n particles, alternately at A and at B of the two-wall case, jittered by a few millimetres."""
    rng = np.random.default_rng(2)
    p = np.zeros(n, bl.PARTICLE_DTYPE)
    at = c["poses"][np.arange(n) % 2]
    p["x"] = (at[:, 0] + rng.uniform(-0.004, 0.004, n)).astype(np.float32)
    p["y"] = (at[:, 1] + rng.uniform(-0.004, 0.004, n)).astype(np.float32)
    p["theta"] = at[:, 2]
    for f in ("x", "y", "theta"):
        p["p_" + f] = p[f]
    p["weight"] = 1.0 / n
    return p


def test_cpp_model_and_filter_equal_the_python_path(gpu_ctx):
    c = bc.two_walls()
    h, w = c["cells"].shape
    prm = c["params"]
    n = 200
    cloud = _split_cloud(c, n)
    with tempfile.TemporaryDirectory() as td:
        exe = _build(td, "beam_model_test")
        inp, outp = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(inp, "wb") as f:
            f.write(struct.pack("<iifff", w, h, float(c["mpc"]), float(c["origin"][0]), float(c["origin"][1])))
            f.write(c["cells"].tobytes())
            f.write(struct.pack("<8f4iq", prm["max_range"], prm["sigma_cells"], prm["z_hit"], prm["z_short"], prm["z_max"], prm["z_rand"], prm["lam"],
                                prm["blocked_factor"], prm["occ_min"], prm["hit_cut"], prm["ray_stride"], 0, prm["span"]))
            f.write(struct.pack("<i", len(c["ranges"])) + c["ranges"].tobytes() + c["thetas"].tobytes())
            f.write(struct.pack("<i", len(c["poses"])) + c["poses"].tobytes())
            f.write(struct.pack("<i", n) + cloud.tobytes())
        r = subprocess.run([exe, inp, outp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 0 and b"beam_model_test ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
        raw = open(outp, "rb").read()
    # the Python path and the model
    beam = bl.BeamModel(ctx=gpu_ctx, **{k: prm[k] for k in KEYS})
    grid = grid_of(gpu_ctx, c)          # (cells_per_meter as the C++ grid forms it from meters_per_cell)
    pf = bl.ParticleFilter(n, ctx=gpu_ctx)
    try:
        t = beam.tables(grid.cpm)
        S = beam.scores(grid, scan_of(c), c["poses"])
        U = beam.units(len(S))
        cast = beam.debug_cast(grid, scan_of(c), c["poses"][0])
        assert np.array_equal(S, bm.scores(c["cells"], c["origin"], c["cpm"], c["ranges"], c["thetas"], c["poses"], prm, t))
        pf.setParticles(cloud)
        est = pf.reweigh_beam(beam, grid, scan_of(c))
        fu = beam.units(n)
        wts = pf.particles()["weight"]
        cl = pf.clusters(0.5, 36, 8)
    finally:
        pf.close()
        beam.close()
        grid.close()
    npos, R = len(c["poses"]), len(cast["p"])
    off = 0
    assert raw[off:off + 1] == b"S"
    assert raw[off + 1:off + 1 + 8 * npos] == S.tobytes() and raw[off + 1 + 8 * npos:off + 1 + 12 * npos] == U.tobytes()
    off += 1 + 12 * npos
    assert raw[off:off + 1] == b"C" and struct.unpack_from("<i", raw, off + 1)[0] == R
    off += 5
    for col in ("first", "K", "z", "zstar"):
        assert np.array_equal(np.frombuffer(raw, np.int32, R, off), cast[col]), col
        off += 4 * R
    assert np.array_equal(np.frombuffer(raw, np.uint32, R, off), cast["p"])
    off += 4 * R
    assert raw[off:off + 1] == b"T" and struct.unpack_from("<5I", raw, off + 1) == (t["rand"], t["max_free"], t["max_blocked"], t["ln2"], t["reach"])
    off += 21
    assert raw[off:off + 1] == b"F"
    ef = struct.unpack_from("<6f", raw, off + 1)
    want = struct.unpack("<3f", struct.pack("<3f", est.x, est.y, est.theta))
    assert ef[:3] == want and ef[3:] == want
    off += 25
    assert raw[off:off + 4 * n] == fu.tobytes() and raw[off + 4 * n:off + 12 * n] == wts.tobytes()
    off += 12 * n
    assert raw[off:off + 1] == b"H"
    have, = struct.unpack_from("<i", raw, off + 1)
    mx, my, share = struct.unpack_from("<3d", raw, off + 5)
    assert raw[off + 29:] == b"E"
    # the reason for the feature, through the filter: the heaviest cluster stands at A and holds nearly all the weight
    A, B = c["poses"]
    assert (fu[0::2] == 2 ** 20).any() and (fu[1::2] == 1).all()
    assert have == 1 and abs(mx - float(A[0])) < 0.01 and abs(my - float(A[1])) < 0.01 and share > 0.999
    assert abs(est.x - float(A[0])) < 0.01 and abs(float(B[0]) - float(A[0])) > 0.9
    assert cl is not None


def _runs(raw):
    """{tag: (iterations, final counts, active, the run's bytes)} of the three runs the binary writes."""
    off, out = 0, {}
    while off < len(raw):
        assert raw[off:off + 1] == b"R"
        tag, start = raw[off + 1:off + 2].decode(), off + 2
        off, its = start, []
        while raw[off:off + 1] == b"I":
            t, x, y, th, a, b, c = struct.unpack_from("<qfffiii", raw, off + 1)
            its.append(((t, x, y, th), (a, b, c)))
            off += 33
        assert raw[off:off + 1] == b"E"
        fin = struct.unpack_from("<iiiii", raw, off + 1)
        active, = struct.unpack_from("<i", raw, off + 21 + 40000)
        off += 21 + 40000 + 4
        out[tag] = (its, fin, active, raw[start:off - 4])
    return out


def test_driver_off_is_untouched_and_on_tracks(maps, tmp_path):
    m, poses, ev = drv._events(maps, mode=1, steps=16, name="convex_10mx10m_5cm", start=(0.0, 0.0, 0.0))
    ev = [e for e in ev if e[0] in "OL"]
    mapfile = str(tmp_path / "convex.map")
    drv._write_map_file(mapfile, m)
    with tempfile.TemporaryDirectory() as td:
        exe = _build(td, "beam_driver_test")
        script, outp = os.path.join(td, "s.bin"), os.path.join(td, "o.bin")
        drv._write_script(script, 1, 1000, ev)
        out = subprocess.check_output([exe, script, outp, mapfile], stderr=subprocess.DEVNULL, timeout=120).decode()
        assert "beam_driver_test ok" in out
        runs = _runs(open(outp, "rb").read())
    assert sorted(runs) == ["B", "n", "o"]
    assert runs["n"][3] == runs["o"][3]                                   # byte for byte: poses, bookkeeping, map
    its0, fin0, act0, _ = runs["n"]
    its1, fin1, act1, _ = runs["B"]
    assert act0 == 0 and runs["o"][2] == 0 and act1 == 1
    assert [(a[0][0], a[1]) for a in its0] == [(b[0][0], b[1]) for b in its1] and fin0 == fin1 and len(its1) >= 12
    assert [a[0] for a in its0] != [b[0] for b in its1]                   # the beam-weighted pose is another pose
    last = its1[-1][0]
    truth = (poses[-1][0] - poses[0][0], poses[-1][1] - poses[0][1])
    print("last pose with the beam model", last[1:], "without", its0[-1][0][1:], "truth", truth)
    assert abs(last[1] - truth[0]) < 0.10 and abs(last[2] - truth[1]) < 0.10   # the bound of the localization-only driver test
