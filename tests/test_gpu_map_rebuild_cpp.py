"""OccupancyGridSLAMT::setScanHistory / rebuildMap and ScanHistoryT (include/botlab/slam_driver.hpp, map_rebuild.hpp), built with
g++ -std=c++11 from tests/cpp/map_rebuild_driver_test.cpp:

  * the driver with the switch never touched and with setScanHistory(0) writes the same bytes;
  * with it on, the history holds the scan and the pose bits of every map update, and rebuildMap() reproduces the live SLAM map byte
    for byte after 16 steps -- the live map IS sequential updates at the recorded poses, so a difference is a bug in the log or the kernel;
  * rebuildMap(truth) equals a mapping-only run at the true poses."""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import test_gpu_slam_driver as drv

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELLS = 200 * 200


def _build(td, name):
    exe = os.path.join(td, name)
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", name + ".cpp"),
                           "-L" + os.path.join(ROOT, "botlab_amd"), "-lbotlab_hip", "-Wl,-rpath," + os.path.join(ROOT, "botlab_amd"), "-o", exe])
    return exe


def _poses(raw, off, n):
    out = [struct.unpack_from("<qfff", raw, off + 20 * i) for i in range(n)]
    return out, off + 20 * n


def _parse(raw):
    """({tag: (iterations, final counts, map, the run's bytes)}, history size, recorded poses, mapped poses, rebuilt map, map at the truth)."""
    off, runs = 0, {}
    while raw[off:off + 1] == b"R":
        tag, start = raw[off + 1:off + 2].decode(), off + 2
        off, its = start, []
        while raw[off:off + 1] == b"I":
            t, x, y, th, a, b, c = struct.unpack_from("<qfffiii", raw, off + 1)
            its.append(((t, x, y, th), (a, b, c)))
            off += 33
        assert raw[off:off + 1] == b"E"
        fin = struct.unpack_from("<iiiii", raw, off + 1)
        cells = np.frombuffer(raw, np.int8, CELLS, off + 21).reshape(200, 200)
        off += 21 + CELLS
        runs[tag] = (its, fin, cells, raw[start:off])
    assert raw[off:off + 1] == b"h"
    held, = struct.unpack_from("<i", raw, off + 1)
    recorded, off = _poses(raw, off + 5, held)
    nm, = struct.unpack_from("<i", raw, off)
    mapped, off = _poses(raw, off + 4, nm)
    assert raw[off:off + 1] == b"r"
    rebuilt = np.frombuffer(raw, np.int8, CELLS, off + 1).reshape(200, 200)
    off += 1 + CELLS
    assert raw[off:off + 1] == b"t"
    at_truth = np.frombuffer(raw, np.int8, CELLS, off + 1).reshape(200, 200)
    assert off + 1 + CELLS == len(raw)
    return runs, held, recorded, mapped, rebuilt, at_truth


def test_driver_history_off_is_untouched_and_rebuild_reproduces_the_live_map(maps):
    _, _, ev_slam = drv._events(maps, mode=3, steps=16)
    _, _, ev_map = drv._events(maps, mode=0, steps=16)
    assert [e[1].ranges.tobytes() for e in ev_slam if e[0] == "L"] == [e[1].ranges.tobytes() for e in ev_map if e[0] == "L"]
    with tempfile.TemporaryDirectory() as td:
        exe = _build(td, "map_rebuild_driver_test")
        s_slam, s_map, outp = os.path.join(td, "s.bin"), os.path.join(td, "m.bin"), os.path.join(td, "o.bin")
        drv._write_script(s_slam, 3, 1000, ev_slam)
        drv._write_script(s_map, 0, 200, ev_map)
        r = subprocess.run([exe, s_slam, s_map, outp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 0 and b"map_rebuild_driver_test ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
        print(r.stdout.decode().strip())
        runs, held, recorded, mapped, rebuilt, at_truth = _parse(open(outp, "rb").read())
    assert sorted(runs) == ["H", "M", "n", "o"]
    assert runs["n"][3] == runs["o"][3]                                   # byte for byte: poses, bookkeeping, map
    its, fin, live, _ = runs["H"]
    assert fin[2] == held == len(mapped) >= 14 and len(its) >= 14         # one entry per map update
    assert recorded == mapped                                             # the pose bits the map was updated with
    assert (live != 0).sum() > 500 and np.array_equal(rebuilt, live), f"{(rebuilt != live).sum()} cells differ"
    truth_map = runs["M"][2]
    assert runs["M"][1][2] == held and (truth_map != 0).sum() > 500
    assert np.array_equal(at_truth, truth_map), f"{(at_truth != truth_map).sum()} cells differ"
    assert not np.array_equal(truth_map, live)
