#!/usr/bin/env python3
"""Regenerates tests/golden/ref_math_vectors.npz: the outputs of the reference's own angle_functions.hpp and interpolation.hpp
(compiled into oracle/_ref/libref_math.so by `make -C oracle` where the reference checkout lies) on the seeded inputs of
tests/helpers.py ref_math_inputs().  Runs only where that library was built; the output is committed, so that
tests/test_oracle_pins.py pins the oracle's restatement of these functions on every machine."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import helpers  # noqa: E402
import oracle_lib  # noqa: E402


def main():
    ref = oracle_lib.load_ref_math()
    if ref is None:
        raise SystemExit("oracle/_ref/libref_math.so is not built: run `make -C oracle` where the reference checkout lies")
    inp = helpers.ref_math_inputs()
    wrap = np.array([ref.ref_wrap_to_pi(a) for a in inp["angles"]], np.float32)
    diff = np.array([ref.ref_angle_diff(l, r) for l, r in inp["pairs"]], np.float64)
    asum = np.array([ref.ref_angle_sum(l, r) for l, r in inp["pairs"]], np.float64)
    n = len(inp["t"])
    o_utime, o_xyt = np.zeros(n, np.int64), np.zeros((n, 3), np.float32)
    for i in range(n):
        b = oracle_lib.OPose(int(inp["b_utime"][i]), *[float(v) for v in inp["b_xyt"][i]])
        e = oracle_lib.OPose(int(inp["e_utime"][i]), *[float(v) for v in inp["e_xyt"][i]])
        o = oracle_lib.OPose()
        ref.ref_interpolate_pose(int(inp["t"][i]), C.byref(b), C.byref(e), C.byref(o))
        o_utime[i], o_xyt[i] = o.utime, (o.x, o.y, o.theta)
    np.savez_compressed(os.path.join(HERE, "ref_math_vectors.npz"), inputs_sha256=np.array(helpers.ref_math_inputs_digest(inp)),
                        wrap_to_pi=wrap, angle_diff=diff, angle_sum=asum, interp_utime=o_utime, interp_xyt=o_xyt)


if __name__ == "__main__":
    main()
