"""The order of the finish's wave-wide scans on DPP (bl_mcl_finish.h: MCLF_DPP_STEPS), restated in numpy.

The steps are read from the header itself: row shifts by 1, 2, 4, 8 inside the 16-lane rows, then the broadcast of lane 15 of a
row into the next one (rows 1 and 3) and of lane 31 into rows 2 and 3.  A lane that a step gives no source lane keeps its own
value -- the kernels hand it the operation's identity (0 for the sums, the empty run for the records).  Applied to a join
that is associative and NOT commutative (2 x 2 integer matrices), every lane must hold the left-to-right product of lanes 0..l:
the order is the thing that can be wrong."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = (1 << 31) - 1           # products mod a prime: exact in int64


def _steps():
    text = open(os.path.join(ROOT, "botlab_amd", "csrc", "bl_mcl_finish.h")).read()
    body = re.search(r"#define MCLF_DPP_STEPS\(STEP\)\s*\\\n(.*)\n", text).group(1)
    return [(int(c, 16), int(r, 16)) for c, r in re.findall(r"STEP\((0x[0-9a-f]+),\s*(0x[0-9a-f]+)\)", body)]


def source_lane(ctrl, row_mask, lane):
    """The lane a DPP control reads for `lane`, or None (no source lane, or the lane's row is outside the row mask)."""
    row = lane >> 4
    if not (row_mask >> row) & 1:
        return None
    if 0x111 <= ctrl <= 0x11f:                      # row_shr:n
        n = ctrl & 0xf
        return lane - n if (lane & 15) >= n else None
    if ctrl == 0x142:                               # row_bcast:15: lane 15 of the row before
        return 16 * row - 1 if row > 0 else None
    if ctrl == 0x143:                               # row_bcast:31: lane 31 into the rows behind it
        return 31 if row >= 2 else None
    raise AssertionError(hex(ctrl))


def dpp_scan(values, join, steps):
    """values: one per lane.  join(earlier, later).  Every step reads the values as they stood before it, like the hardware."""
    v = list(values)
    for ctrl, row_mask in steps:
        before = list(v)
        for lane in range(64):
            s = source_lane(ctrl, row_mask, lane)
            if s is not None:
                v[lane] = join(before[s], before[lane])
    return v


def _matmul(a, b):
    return (a.astype(np.int64) @ b.astype(np.int64)) % P


def test_steps_are_the_ones_the_model_knows():
    assert _steps() == [(0x111, 0xf), (0x112, 0xf), (0x114, 0xf), (0x118, 0xf), (0x142, 0xa), (0x143, 0xc)]


def test_every_lane_holds_the_left_to_right_product():
    steps = _steps()
    rng = np.random.default_rng(7)
    for trial in range(8):
        mats = [rng.integers(1, P, (2, 2)) for _ in range(64)]
        got = dpp_scan(mats, _matmul, steps)
        run = None
        for lane in range(64):
            run = mats[lane] if run is None else _matmul(run, mats[lane])
            assert np.array_equal(got[lane], run), (trial, lane)


def test_the_join_is_not_commutative_and_the_test_sees_a_swapped_order():
    steps = _steps()
    rng = np.random.default_rng(8)
    mats = [rng.integers(1, P, (2, 2)) for _ in range(64)]
    got = dpp_scan(mats, lambda earlier, later: _matmul(later, earlier), steps)
    run = mats[0]
    wrong = 0
    for lane in range(1, 64):
        run = _matmul(run, mats[lane])
        wrong += int(not np.array_equal(got[lane], run))
    assert wrong == 63


def test_sums_and_last_lane_total():
    steps = _steps()
    rng = np.random.default_rng(9)
    units = [int(u) for u in rng.integers(0, 1 << 32, 64)]
    got = dpp_scan(units, lambda a, b: a + b, steps)
    assert got == [int(c) for c in np.cumsum(np.array(units, dtype=object))]
    assert got[63] == sum(units)                    # what the all-reduce reads from lane 63


def test_every_lane_is_reached_from_every_earlier_lane_once():
    """Sets of lane numbers under union-with-count: lane l ends with exactly {0..l}, no lane joined twice."""
    steps = _steps()
    got = dpp_scan([[l] for l in range(64)], lambda a, b: a + b, steps)
    for lane in range(64):
        assert got[lane] == list(range(lane + 1)), lane
