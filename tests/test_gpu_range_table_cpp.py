"""RangeTableT (include/botlab/range_table.hpp), the table forms of BeamModelT and ParticleFilterT and
OccupancyGridSLAMT::setBeamRangeTable, built with g++ -std=c++11 from tests/cpp/range_table_test.cpp:

  * info, directions, table, scoresTable, units, debugLookup, reweighBeamTable and reweighTable equal the Python path byte for byte;
  * the driver with the switch never touched and with setBeamRangeTable(false) writes the same bytes, with the beam model off and on;
  * with both switches on and a map from a file it builds exactly one table, reads it for every reweigh until its first map update (the
    first iteration of a localization-only run; all of a global search) and for none after it, and still tracks the truth."""
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
HN = 128


def test_cpp_classes_equal_the_python_path(gpu_ctx):
    c = bc.two_walls()
    h, w = c["cells"].shape
    prm = c["params"]
    n = 200
    cloud = _split_cloud(c, n)
    with tempfile.TemporaryDirectory() as td:
        exe = _build(td, "range_table_test")
        inp, outp = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(inp, "wb") as f:
            f.write(struct.pack("<iifff", w, h, float(c["mpc"]), float(c["origin"][0]), float(c["origin"][1])))
            f.write(c["cells"].tobytes())
            f.write(struct.pack("<8f4iq", prm["max_range"], prm["sigma_cells"], prm["z_hit"], prm["z_short"], prm["z_max"], prm["z_rand"], prm["lam"],
                                prm["blocked_factor"], prm["occ_min"], prm["hit_cut"], prm["ray_stride"], 0, prm["span"]))
            f.write(struct.pack("<i", HN))
            f.write(struct.pack("<i", len(c["ranges"])) + c["ranges"].tobytes() + c["thetas"].tobytes())
            f.write(struct.pack("<i", len(c["poses"])) + c["poses"].tobytes())
            f.write(struct.pack("<i", n) + cloud.tobytes())
        r = subprocess.run([exe, "model", inp, outp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 0 and b"range_table_test ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
        raw = open(outp, "rb").read()
    beam = bl.BeamModel(ctx=gpu_ctx, **{k: prm[k] for k in KEYS})
    grid = grid_of(gpu_ctx, c)
    rt = bl.RangeTable(gpu_ctx, HN)
    pf = bl.ParticleFilter(n, ctx=gpu_ctx)
    try:
        rt.build(beam, grid)
        info, D, T = rt.info(), rt.directions(), rt.read()
        S = beam.scores_table(rt, scan_of(c), c["poses"])
        U = beam.units(len(S))
        look = beam.debug_lookup(rt, scan_of(c), c["poses"][0])
        pf.setParticles(cloud)
        est = pf.reweigh_beam_table(beam, rt, scan_of(c))
        fu = beam.units(n)
        wts = pf.particles()["weight"]
    finally:
        pf.close()
        rt.close()
        beam.close()
        grid.close()
    npos, R = len(c["poses"]), len(look["p"])
    assert raw[0:1] == b"I" and struct.unpack_from("<6iq", raw, 1) == tuple(info[k] for k in ("width", "height", "headings", "reach", "occ_min", "built", "bytes"))
    off = 33
    assert raw[off:off + 1] == b"D" and raw[off + 1:off + 1 + 8 * HN] == D.tobytes()
    off += 1 + 8 * HN
    assert raw[off:off + 1] == b"T" and raw[off + 1:off + 1 + T.nbytes] == T.tobytes()
    off += 1 + T.nbytes
    assert raw[off:off + 1] == b"S"
    assert raw[off + 1:off + 1 + 8 * npos] == S.tobytes() and raw[off + 1 + 8 * npos:off + 1 + 12 * npos] == U.tobytes()
    off += 1 + 12 * npos
    assert raw[off:off + 1] == b"C" and struct.unpack_from("<i", raw, off + 1)[0] == R
    off += 5
    for col in ("h", "z", "zstar"):
        assert np.array_equal(np.frombuffer(raw, np.int32, R, off), look[col]), col
        off += 4 * R
    assert np.array_equal(np.frombuffer(raw, np.uint32, R, off), look["p"])
    off += 4 * R
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
    """{tag: (iterations, final counts, (active, builds, reweighs), the run's bytes)} of the runs the binary writes."""
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
        tail = struct.unpack_from("<iii", raw, off + 21 + 40000)
        off += 21 + 40000 + 12
        out[tag] = (its, fin, tail, raw[start:off - 12])
    return out


def test_driver_off_is_untouched_and_on_builds_one_table(maps, tmp_path):
    m, poses, ev = drv._events(maps, mode=1, steps=16, name="convex_10mx10m_5cm", start=(0.0, 0.0, 0.0))
    ev = [e for e in ev if e[0] in "OL"]
    mapfile = str(tmp_path / "convex.map")
    drv._write_map_file(mapfile, m)
    with tempfile.TemporaryDirectory() as td:
        exe = _build(td, "range_table_test")
        script, outp = os.path.join(td, "s.bin"), os.path.join(td, "o.bin")
        drv._write_script(script, 1, 1000, ev)
        out = subprocess.check_output([exe, "driver", script, outp, mapfile], stderr=subprocess.DEVNULL, timeout=180).decode()
        assert "range_table_test ok" in out
        runs = _runs(open(outp, "rb").read())
    assert sorted(runs) == ["B", "G", "T", "b", "n", "o"]
    assert runs["n"][3] == runs["o"][3] and runs["B"][3] == runs["b"][3]   # byte for byte: poses, bookkeeping, map
    assert runs["n"][3] != runs["B"][3]
    for tag in "noBb":
        assert runs[tag][2] == ((1 if tag in "Bb" else 0), 0, 0)
    itsB, finB, _, _ = runs["B"]
    itsT, finT, tailT, _ = runs["T"]
    # localization-only: the driver extends its map at the end of every iteration, so only the first reweigh may read the table
    assert tailT == (1, 1, 1) and itsT[0][1][2] == 1
    assert [(a[0][0], a[1]) for a in itsB] == [(b[0][0], b[1]) for b in itsT] and finB == finT and len(itsT) >= 12
    last = itsT[-1][0]
    truth = (poses[-1][0] - poses[0][0], poses[-1][1] - poses[0][1])
    print("last pose with the table", last[1:], "with the cast", itsB[-1][0][1:], "truth", truth)
    assert abs(last[1] - truth[0]) < 0.10 and abs(last[2] - truth[1]) < 0.10   # the bound of the localization-only driver test
    # global localization: every searching iteration leaves the map alone and reads the one table
    itsG, _, tailG, _ = runs["G"]
    searching = next((i for i, it in enumerate(itsG) if it[1][2] > 0), len(itsG) - 1) + 1
    print("global search: iterations", len(itsG), "that read the table", tailG[2], "map updates at the end", itsG[-1][1][2])
    assert tailG[0] == 1 and tailG[1] == 1 and tailG[2] == searching >= 1
