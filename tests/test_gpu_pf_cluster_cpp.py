"""ParticleFilterT::clusters and heaviestCluster (include/botlab/botlab_dropin.hpp), built with g++ -std=c++11 from
tests/cpp/pf_cluster_test.cpp, on the bimodal cloud of tests/pf_cluster_cases.py: the clusters and labels equal the integer model,
the heaviest cluster holds exactly 0.7 of the weight and sits on A, while the spread of the whole cloud is far above the
driver's tolerance."""
import ctypes as C
import math
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import pf_cluster_cases as cases
import pf_cluster_model as pm
from botlab_amd import _capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bimodal_through_the_drop_in():
    c = cases.bimodal()
    n, K = len(c["x"]), 8
    mod = pm.clusters(c["x"], c["y"], c["th"], c["units"], c["bin_xy"], c["T"], K)
    with tempfile.TemporaryDirectory() as td:
        exe, inp, outp = os.path.join(td, "pf_cluster_test"), os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "pf_cluster_test.cpp"),
                               "-L" + os.path.join(ROOT, "botlab_amd"), "-lbotlab_hip", "-Wl,-rpath," + os.path.join(ROOT, "botlab_amd"), "-o", exe])
        with open(inp, "wb") as f:
            f.write(struct.pack("<i", n))
            rec = np.zeros(n, np.dtype([("x", "<f4"), ("y", "<f4"), ("th", "<f4"), ("u", "<u4")]))
            rec["x"], rec["y"], rec["th"], rec["u"] = c["x"], c["y"], c["th"], c["units"]
            f.write(rec.tobytes())
            f.write(struct.pack("<dii", c["bin_xy"], c["T"], K))
        out = subprocess.check_output([exe, inp, outp], timeout=120).decode()
        assert "pf_cluster_test ok" in out
        raw = open(outp, "rb").read()
    res = _capi.PfClusters.from_buffer_copy(raw[:9240])
    labels = np.frombuffer(raw, np.int32, n, 9240)
    off = 9240 + 4 * n
    has, = struct.unpack_from("<i", raw, off)
    pose = _capi.PfClusterPose.from_buffer_copy(raw[off + 4:off + 68])
    spread = _capi.PfSpread.from_buffer_copy(raw[off + 68:off + 148])
    assert (res.num_clusters, res.units_sum, res.active) == (mod["num_clusters"], mod["units_sum"], n)
    for k, e in enumerate(mod["clusters"][:K]):
        g = res.clusters[k]
        assert (g.count, g.units, (g.anchor_ix, g.anchor_iy, g.anchor_it)) == (e["count"], e["units"], e["anchor"])
        for s in pm.SUMS:
            assert getattr(g, s).value() == e[s], (k, s)
    assert np.array_equal(labels, mod["labels"])
    assert has == 1 and pose.share == 0.7 and res.clusters[0].units * 10 == res.units_sum * 7
    want = pm.cluster_pose(mod["clusters"][0], mod["units_sum"], c["bin_xy"])
    assert {f: getattr(pose, f) for f, _ in _capi.PfClusterPose._fields_} == want
    assert abs(pose.mean_x - 1.0) < 0.01 and abs(pose.mean_y - 2.0) < 0.01 and abs(pose.theta - 0.5) < 0.02
    h = 0.5 * (spread.var_x + spread.var_y)
    assert math.sqrt(h + math.sqrt(0.25 * (spread.var_x - spread.var_y) ** 2 + spread.cov_xy ** 2)) > 0.2      # the driver's default tolerance
    assert 1.5 < spread.mean_x < 4.5                          # the whole cloud's mean lies between the modes
