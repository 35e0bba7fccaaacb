"""The step stream of the obstacle tracks' C++ programs (tests/cpp/obstacle_tracks_stream.hpp): a script of
tests/test_obstacle_tracks_model_cpu.py written as their input, and their output read back and held against the model's results."""
import struct

import numpy as np

import obstacle_tracks_model as tm


def robot_pose(script, cell):
    """The middle of a cell, in metres (float32)."""
    return (np.float32(float(script.origin[0]) + (cell[0] + 0.5) * float(script.mpc)), np.float32(float(script.origin[1]) + (cell[1] + 0.5) * float(script.mpc)))


def encode(script, model, refused_compose=True):
    """(bytes, the indices of the steps sent).  refused_compose False: the composes that the model refuses are left out."""
    w, h = script.shape
    lp, tp = script.layer, script.params
    out = [struct.pack("<iifff", w, h, float(script.mpc), float(script.origin[0]), float(script.origin[1])), script.cells.tobytes(),
           struct.pack("<fiiii", lp["max_range"], lp["occ_min"], lp["tol_cells"], lp["ttl_scans"], lp["min_hits"]),
           struct.pack("<8i", *[tp[k] for k in tm.PARAM_NAMES])]
    sent = []
    params = dict(tp)
    for k, st in enumerate(script.steps):
        if st[0] == "layer":
            out.append(b"L" + st[1].tobytes() + st[2].tobytes() + struct.pack("<I", st[3]))
        elif st[0] == "update":
            out.append(b"U")
        elif st[0] == "reset":
            out.append(b"R")
        elif st[0] == "roundtrip":
            out.append(b"T")
        elif st[0] == "upload":
            out.append(b"S" + np.ascontiguousarray(st[1], dtype=tm.TRACK_DTYPE).tobytes() + struct.pack("<IIii", st[2], st[3], int(st[4]), 0))
        elif st[0] == "params":
            p = dict(params, **st[1])
            if model[k][0] == "ok":
                params = p
            out.append(b"P" + struct.pack("<8i", *[p[name] for name in tm.PARAM_NAMES]))
        elif st[0] == "compose":
            if model[k][0] != "ok" and not refused_compose:
                continue
            x, y = robot_pose(script, st[2])
            out.append(b"C" + struct.pack("<iffi", st[1], x, y, st[3]))
        else:
            raise AssertionError(st[0])
        sent.append(k)
    out.append(b"E")
    return b"".join(out), sent


def check(raw, script, model, sent, distances=False):
    """Everything in the programs' output equals the model.  Returns [(step, composed, distances or None)] of the accepted composes."""
    w, h = script.shape
    off, composes = 0, []
    tags = dict(layer=b"L", update=b"U", reset=b"R", roundtrip=b"T", upload=b"S", params=b"P", compose=b"C")
    for k in sent:
        st, (res, snap) = script.steps[k], model[k]
        assert raw[off:off + 1] == tags[st[0]], (k, st[0], raw[off:off + 1])
        rc, = struct.unpack_from("<i", raw, off + 1)
        off += 5
        assert (rc == 0) == (res == "ok"), (k, st[0], rc, res)
        if st[0] == "update":
            assert rc == {"ok": 0, "arg": 2, "state": 4}[res], (k, rc, res)
            for key, dtype in (("tracks", tm.TRACK_DTYPE), ("blobs", tm.BLOB_DTYPE), ("labels", np.dtype("<i4"))):
                n, = struct.unpack_from("<i", raw, off)
                got = np.frombuffer(raw, dtype, n, off + 4)
                off += 4 + n * dtype.itemsize
                assert n == len(snap[key]), (k, key, n, len(snap[key]))
                exp = np.ascontiguousarray(snap[key], dtype=dtype)
                assert got.tobytes() == exp.tobytes(), (k, key)
            stats = struct.unpack_from("<II12i", raw, off)
            off += 56
            exp = tuple(snap["stats"][name] for name in tm.STAT_NAMES)
            assert stats[:-1] == exp[:-1] and (not distances or stats[-1] == exp[-1]), (k, stats, exp)   # rounds: the device's only
        elif st[0] == "compose" and rc == 0:
            got = np.frombuffer(raw, np.int8, w * h, off).reshape(h, w)
            off += w * h
            assert np.array_equal(got, snap["composed"]), (k, st)
            d = None
            if distances:
                assert raw[off:off + 1] == b"D"
                d = np.frombuffer(raw, np.float32, w * h, off + 1).reshape(h, w)
                off += 1 + 4 * w * h
            composes.append((k, got, d))
    assert off == len(raw), (off, len(raw))
    return composes
