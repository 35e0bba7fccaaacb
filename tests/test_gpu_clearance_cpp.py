"""ClearanceGridT (include/botlab/clearance_grid.hpp), the leap forms of BeamModelT and ParticleFilterT and
OccupancyGridSLAMT::setBeamLeapCast, built with g++ -std=c++11 from tests/cpp/clearance_test.cpp:

  * info, grid, scoresLeap, units, debugLeap, reweighBeamLeap and reweighLeap equal the Python path byte for byte;
  * the driver with the switch never touched and with setBeamLeapCast(false) writes the same bytes, with the beam model off and on;
  * with the beam model on, a localization-only run, whose map changes at every iteration, writes the same poses, particles and map
    byte for byte with the switch on as with it off; its counters show one build, one update per map update and every reweigh by
    leaps; with the range table on as well the table keeps its turn and the leaps take every reweigh after it, with the bytes of
    the run that casts there; at the end the driver's grid equals a fresh build on the final map."""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import botlab_amd as bl
import beam_cases as bc
import test_gpu_slam_driver as drv
from test_gpu_beam import KEYS, grid_of, scan_of
from test_gpu_beam_cpp import _build, _split_cloud

pytestmark = pytest.mark.gpu
CAP = 7
NP = 1000


def test_cpp_classes_equal_the_python_path(gpu_ctx):
    c = bc.two_walls()
    h, w = c["cells"].shape
    prm = c["params"]
    n = 200
    cloud = _split_cloud(c, n)
    with tempfile.TemporaryDirectory() as td:
        exe = _build(td, "clearance_test")
        inp, outp = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(inp, "wb") as f:
            f.write(struct.pack("<iifff", w, h, float(c["mpc"]), float(c["origin"][0]), float(c["origin"][1])))
            f.write(c["cells"].tobytes())
            f.write(struct.pack("<8f4iq", prm["max_range"], prm["sigma_cells"], prm["z_hit"], prm["z_short"], prm["z_max"], prm["z_rand"], prm["lam"],
                                prm["blocked_factor"], prm["occ_min"], prm["hit_cut"], prm["ray_stride"], 0, prm["span"]))
            f.write(struct.pack("<i", CAP))
            f.write(struct.pack("<i", len(c["ranges"])) + c["ranges"].tobytes() + c["thetas"].tobytes())
            f.write(struct.pack("<i", len(c["poses"])) + c["poses"].tobytes())
            f.write(struct.pack("<i", n) + cloud.tobytes())
        r = subprocess.run([exe, "model", inp, outp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 0 and b"clearance_test ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
        raw = open(outp, "rb").read()
    beam = bl.BeamModel(ctx=gpu_ctx, **{k: prm[k] for k in KEYS})
    grid = grid_of(gpu_ctx, c)
    cl = bl.ClearanceGrid(gpu_ctx, CAP)
    pf = bl.ParticleFilter(n, ctx=gpu_ctx)
    try:
        cl.build(grid, prm["occ_min"])
        info, D = cl.info(), cl.read()
        S = beam.scores_leap(cl, scan_of(c), c["poses"])
        U = beam.units(len(S))
        cast = beam.debug_leap(cl, scan_of(c), c["poses"][0])
        pf.setParticles(cloud)
        est = pf.reweigh_beam_leap(beam, cl, scan_of(c))
        fu = beam.units(n)
        wts = pf.particles()["weight"]
    finally:
        pf.close()
        cl.close()
        beam.close()
        grid.close()
    npos, R = len(c["poses"]), len(cast["p"])
    assert raw[0:1] == b"I"
    assert struct.unpack_from("<6iq", raw, 1) == tuple(info[k] for k in ("width", "height", "cap", "occ_min", "built")) + (0, info["bytes"])
    off = 33
    assert raw[off:off + 1] == b"D" and raw[off + 1:off + 1 + D.nbytes] == D.tobytes()
    off += 1 + D.nbytes
    assert raw[off:off + 1] == b"S"
    assert raw[off + 1:off + 1 + 8 * npos] == S.tobytes() and raw[off + 1 + 8 * npos:off + 1 + 12 * npos] == U.tobytes()
    off += 1 + 12 * npos
    assert raw[off:off + 1] == b"C" and struct.unpack_from("<i", raw, off + 1)[0] == R
    off += 5
    for col in ("first", "K", "z", "zstar", "p", "rounds"):
        assert np.array_equal(np.frombuffer(raw, np.uint32 if col == "p" else np.int32, R, off), cast[col]), col
        off += 4 * R
    assert (cast["rounds"] > 0).all() and (cast["rounds"] <= cast["first"] + 1).all() and cast["rounds"].sum() < (cast["first"] + 1).sum()
    assert raw[off:off + 1] == b"F"
    ef = struct.unpack_from("<9f", raw, off + 1)
    want = struct.unpack("<3f", struct.pack("<3f", est.x, est.y, est.theta))
    assert ef[:3] == want and ef[3:6] == want and ef[6:] == want
    off += 37
    assert raw[off:off + 4 * n] == fu.tobytes() and raw[off + 4 * n:off + 12 * n] == wts.tobytes()
    assert raw[off + 12 * n:] == b"E"
    A, B = c["poses"]
    assert S[0] > S[1] and U.tolist() == [2 ** 20, 1] and (fu[1::2] == 1).all()
    assert abs(est.x - float(A[0])) < 0.01 and abs(float(B[0]) - float(A[0])) > 0.9


def _runs(raw):
    """{tag: (iterations, final counts, tail, the run's bytes)} of the runs the binary writes."""
    off, out = 0, {}
    while off < len(raw):
        assert raw[off:off + 1] == b"R"
        tag, start = raw[off + 1:off + 2].decode(), off + 2
        off, its = start, []
        while raw[off:off + 1] == b"I":
            t, x, y, th, a, b, c = struct.unpack_from("<qfffiii", raw, off + 1)
            its.append(((t, x, y, th), (a, b, c)))
            off += 33
            assert raw[off:off + 1] == b"P"
            off += 1 + 20 * NP
        assert raw[off:off + 1] == b"E"
        fin = struct.unpack_from("<iiiii", raw, off + 1)
        tail = struct.unpack_from("<6i", raw, off + 21 + 40000)
        off += 21 + 40000 + 24
        out[tag] = (its, fin, tail, raw[start:off - 24])
    return out


def test_driver_off_is_untouched_and_on_leaves_the_casts_bytes(maps, tmp_path):
    m, poses, ev = drv._events(maps, mode=1, steps=16, name="convex_10mx10m_5cm", start=(0.0, 0.0, 0.0))
    ev = [e for e in ev if e[0] in "OL"]
    mapfile = str(tmp_path / "convex.map")
    drv._write_map_file(mapfile, m)
    with tempfile.TemporaryDirectory() as td:
        exe = _build(td, "clearance_test")
        script, outp = os.path.join(td, "s.bin"), os.path.join(td, "o.bin")
        drv._write_script(script, 1, NP, ev)
        out = subprocess.check_output([exe, "driver", script, outp, mapfile], stderr=subprocess.DEVNULL, timeout=180).decode()
        assert "clearance_test ok" in out
        runs = _runs(open(outp, "rb").read())
    assert sorted(runs) == ["B", "L", "T", "b", "n", "o", "t"]
    assert runs["n"][3] == runs["o"][3] and runs["B"][3] == runs["b"][3]   # byte for byte: poses, particles, bookkeeping, map
    assert runs["n"][3] != runs["B"][3]
    for tag in "noBb":
        assert runs[tag][2] == ((1 if tag in "Bb" else 0), 0, 0, 0, 0, -1)
    # the switch on: the cast's bytes, by leaps
    assert runs["L"][3] == runs["B"][3]
    assert runs["T"][3] == runs["t"][3]                                       # behind the range table's turn too (whose own bytes are not the cast's)
    assert runs["t"][2] == (1, 0, 0, 0, 1, -1)
    itsL, finL, tailL, _ = runs["L"]
    counts = [it[1][2] for it in itsL]
    map_updates = finL[2]
    # every iteration that localizes ends with a map update (an iteration without a pose for its scan does neither)
    assert map_updates >= 12 and counts[0] <= 1 and counts[-1] == map_updates and all(0 <= b - a <= 1 for a, b in zip(counts, counts[1:]))
    print("iterations", len(itsL), "map updates", map_updates, "tail L", tailL, "tail T", runs["T"][2])
    assert tailL == (1, 1, map_updates, map_updates, 0, 1)                    # one build, an update per map update, every reweigh by leaps
    # the table's turn first, on the map as loaded; the grid is built on the map after the first update and follows the rest
    assert runs["T"][2] == (1, 1, map_updates - 1, map_updates - 1, 1, 1)
