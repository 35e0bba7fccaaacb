"""The list form of the finish's chain (bl_mcl_finish.h: mclf_chain, mclf_replay_table) on chains of the shapes its entry pipeline can
get wrong: the accumulator travels as (key, M), entry k + 1's step and table rows are read while entry k is computed, and the first
leaving term's data is fetched by one ballot and independent lane reads.

Two kinds of input, every result held bit for bit against the oracle:
  * SENSOR UPDATES -- N = 1 281 (one record past the pre-chain's nine sub-tiles: a list of at most two entries), 2 560, 8 192 and
    20 000 particles on the shipped 200 x 200 map, on the five clouds of tests/test_gpu_finish_scans.py, riding in k_map_update and
    alone (k_mcl_finish): the pose, the particles, the next update's source indices (they come from the weight prefix), and the chain
    statistics where they say something.
  * UPLOADS (bl_pf_set_particles + the on-demand estimate, k_mcl_finish alone: an upload has no update for a map launch to finish) --
    8 192 particles of equal units, so that every weight is exactly 2^-13 and every term x / 8192 is exact: sequences built term by
    term to put a leaving term, a tie or a wrong prediction at a chosen index of a chosen sub-tile.
Before anything runs on the GPU, `census` walks the oracle's own serially rounded partial sums (and the double-precision prefix sums
the kernels predict with) on the CPU and names the shapes each input holds; test_the_inputs_hold_every_shape asserts that every shape
listed in SHAPES occurs.  A sub-tile is 128 consecutive particles; the chain proper starts behind the ninth."""
import ctypes as C

import numpy as np
import pytest

import botlab_amd as bl
import helpers
import oracle_lib
import resample_rule_model as rrm
import test_gpu_finish_scans as fs
from botlab_amd.host import PARTICLE_DTYPE

pytestmark = pytest.mark.gpu

SUB = 128                   # MCLF_SUB
PRE = 9                     # MCLF_PRE_SUBS
BATCH = 64                  # records per staged batch
MAXENT = 32                 # MCLF_MAXENT
MARGIN = 4096               # MCLF_MARGIN
MLO, MHI = 1 << 23, 1 << 24

SIZES = [1281, 2560, 8192, 20_000]
UPDATE_CASES = [(n, c) for n in SIZES for c in fs.CLOUDS]

SHAPES = ("entry_is_last_subtile", "short_last_subtile", "two_risky_in_a_batch", "table_key_is_not_the_accumulators", "second_column_fails",
          "leaves_twice", "stayed_inside", "leaves_at_0", "leaves_at_even_index", "leaves_at_last", "arrives_at_2_24", "wild_fits", "wild_misses")


# ---------------------------------------------------------------------------------------------------------------- CPU side
def _key(bits):
    ex = (bits >> 23) & 0xFF
    return np.where((ex < 16) | (ex == 255), 0, 0x400 | ((bits >> 31) << 9) | ex).astype(np.int64)


def _mag(bits):
    return ((bits & 0x7FFFFF) | 0x800000).astype(np.int64)


def serial_sum(t):
    """bits of the reference's accumulator behind every term: acc <- fl32(fl64(acc + t_i))"""
    acc = np.float32(0.0)
    out = np.empty(len(t), np.float32)
    for i, v in enumerate(t):
        acc = np.float32(np.float64(acc) + v)
        out[i] = acc
    return out


def census(t):
    """Shapes of one axis' chain, from its terms t (float64, in particle order)."""
    N = len(t)
    acc = serial_sum(t)
    bits = acc.view(np.uint32).astype(np.int64)
    key, mag = _key(bits), _mag(bits)
    kb = np.concatenate([[0], key[:-1]])                         # the key in front of term i
    pred = np.cumsum(t)                                          # what a double-precision prefix sum predicts behind term i
    pkey = _key(np.asarray(pred, np.float32).view(np.uint32).astype(np.int64))
    pkb = np.concatenate([[0], pkey[:-1]])
    # a step that ties: fl64(acc + t) lies midway between two floats
    prev = np.concatenate([[np.float32(0)], acc[:-1]]).astype(np.float64)
    r = prev + t
    r32 = r.astype(np.float32)
    tie = (r != r32.astype(np.float64)) & (np.abs(r32.astype(np.float64) - r) * 2 == np.abs(np.spacing(r32).astype(np.float64)))
    found = set()
    nsub = (N + SUB - 1) // SUB
    if N % SUB:
        found.add("short_last_subtile")
    risky_subs = []
    for s in range(PRE, nsub):
        lo, hi = s * SUB, min(s * SUB + SUB, N)
        leave = np.nonzero(key[lo:hi] != kb[lo:hi])[0]
        up = [j for j in leave if kb[lo + j] != 0 and key[lo + j] == kb[lo + j] + 1]
        # a term too large for a record of the binade in front of the sub-tile (a quarter of its lower end and more), or one that ties
        oversized = kb[lo] != 0 and bool(np.any(np.abs(t[lo:hi]) >= 2.0 ** (int(kb[lo] & 0xFF) - 128)))
        wildish = any(j not in up for j in leave) or len(leave) >= 2 or bool(np.any(key[lo:hi] == 0)) or kb[lo] == 0 or oversized
        near = len(leave) == 0 and not oversized and kb[lo] != 0 and (
            min(int(mag[lo:hi].min()), int(mag[lo - 1])) - MLO < MARGIN // 2 or MHI - max(int(mag[lo:hi].max()), int(mag[lo - 1])) < MARGIN // 2)
        if len(leave) or near or oversized:
            risky_subs.append(s)
        if near:
            found.add("stayed_inside")
        if len(leave) == 0 and not oversized:
            continue
        if s == nsub - 1:
            found.add("entry_is_last_subtile")
        if kb[lo] != 0 and pkb[lo] != 0 and kb[lo] != pkb[lo]:
            found.add("table_key_is_not_the_accumulators")
        j = int(leave[0]) if len(leave) else -1
        if not wildish:
            found.add("leaves_at_0" if j == 0 else "leaves_at_last" if j == hi - lo - 1 else "leaves_at_even_index" if j % 2 == 0 else "leaves_inside")
            if len(leave) == 1 and mag[lo + j] == MLO:
                found.add("arrives_at_2_24")                     # the exact step lands on the next binade's first value
            if len(leave) == 1 and np.any(tie[lo + j + 1:hi]):
                found.add("second_column_fails")                 # a tie in the next binade, behind the crossing
        if len(leave) >= 2:
            found.add("leaves_twice")
        if wildish:
            same = kb[lo] == pkb[lo] and np.array_equal(key[lo:hi], pkey[lo:hi]) and not np.any(tie[lo:hi])
            found.add("wild_fits" if same else "wild_misses")
    for a, b in zip(risky_subs, risky_subs[1:]):
        if a // BATCH == b // BATCH:
            found.add("two_risky_in_a_batch")
    return found, risky_subs


# ---------------------------------------------------------------------------------------------------------------- uploads
UP_N = 8192                 # equal units: every weight is exactly 2^-13


def _pairs(first_sub, count, big):
    """zeros behind the pre-chain's ones, and in `count` consecutive sub-tiles from `first_sub` a term +big then -big: too large for
    a record (a quarter of the binade and more), so each of these sub-tiles is risky and goes by a wild map"""
    v = np.zeros(UP_N, np.float32)
    v[:PRE * SUB] = 1.0
    for s in range(first_sub, first_sub + count):
        v[s * SUB + 5], v[s * SUB + 6] = big, -big
    return v


def _ones_behind_zeros(zeros):
    v = np.ones(UP_N, np.float32)
    v[:zeros] = 0.0
    return v


def upload_sets():
    """name -> (x, y) float32 sequences for UP_N particles of equal units (term i = value / 8192, exact)."""
    sets = {}
    # ones: the sum is (i + 1) / 8192, exact.  It reaches 0.25, 0.5 and 1.0 with the LAST term of sub-tiles 15, 31 and 63 (the last
    # one), each time exactly the next binade's first value; sub-tiles 16 and 32 start on a binade's first value and stay inside.
    # y: exactly MAXENT risky sub-tiles behind the pre-chain -- the longest list there is
    sets["ones_and_full_list"] = (_ones_behind_zeros(0), _pairs(PRE, MAXENT, 512.0))
    # one zero in front: the crossings move to the FIRST term of sub-tiles 16 and 32.  y: one risky sub-tile more -- no list, the walk
    sets["first_term_and_overflow"] = (_ones_behind_zeros(1), _pairs(PRE, MAXENT + 1, 512.0))
    # three zeros in front: the crossings at index 2 (an even index behind the first lane); behind the crossing of 0.5 a term that
    # ties in the binade above (1 + 2^-12 over 8192 = 2^11 + 1/2 ulps there), so the table's second column sends it to the replay.
    x = _ones_behind_zeros(3)
    x[32 * SUB + 10] = np.float32(1.0 + 2.0 ** -12)
    # y: eight terms of a quarter ulp in the pre-chain's last sub-tile (a float drops them, the double prediction keeps them: two
    # ulps apart), then in sub-tile 12 a term that takes the true sum to one ulp below 0.25 and the prediction above it, and back
    y = np.zeros(UP_N, np.float32)
    y[:PRE * SUB] = 1.0
    y[PRE * SUB - 8:PRE * SUB] = np.float32(2.0 ** -15)
    big = np.float32(2048.0 - (PRE * SUB - 8) - 2.0 ** -13)
    y[12 * SUB + 5], y[12 * SUB + 6] = big, -big
    sets["even_index_tie_and_wild_miss"] = (x, y)
    # x: the prediction on the other side of 0.25 from the true sum at the start of sub-tile 16 -- 2031 ones, eight twos, one term
    # of 1 - 2^-13 and eight quarter-ulp terms (in the twos' places) make 0.25 - 1 ulp in a float and 0.25 + 1 ulp in a double; the table is made for the
    # binade above the accumulator's.  y: a sub-tile of terms near 0.01 that crosses 0.5 and 1.0
    x = np.ones(UP_N, np.float32)
    x[8:16] = 2.0
    x[16] = np.float32(1.0 - 2.0 ** -13)
    x[PRE * SUB - 8:PRE * SUB] = np.float32(2.0 ** -15)
    y = np.ones(UP_N, np.float32)
    y[20 * SUB:21 * SUB] = 82.0
    sets["wrong_table_binade_and_twice"] = (x, y)
    return sets


def upload_terms(v):
    units = np.full(UP_N, 1000, np.uint32)
    w = rrm.weights_of(units)
    assert np.all(w == 2.0 ** -13)
    return w * v.astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- shared
@pytest.fixture(scope="module")
def update_sides(oracle, maps):
    """(N, cloud) -> fs.oracle_side(...), computed once"""
    return {(n, c): fs.oracle_side(oracle, maps, n, c) for n, c in UPDATE_CASES}


@pytest.fixture(scope="module")
def shapes(update_sides):
    """input name -> axis -> (shapes, risky sub-tiles by the census)"""
    out = {}
    for (n, c), (_, _, _, _, after) in update_sides.items():
        w = after["weight"].astype(np.float64)
        out[(n, c)] = {ax: census(w * after[ax].astype(np.float64)) for ax in ("x", "y")}
    for name, (x, y) in upload_sets().items():
        out[name] = {"x": census(upload_terms(x)), "y": census(upload_terms(y))}
    return out


def test_the_inputs_hold_every_shape(shapes):
    union = set()
    for per_axis in shapes.values():
        for found, _ in per_axis.values():
            union |= found
    print({k: {ax: (sorted(v[0]), len(v[1])) for ax, v in per.items()} for k, per in shapes.items()})
    assert not [s for s in SHAPES if s not in union], sorted(union)
    # the built sequences are what they were built to be
    up = {k: v for k, v in shapes.items() if isinstance(k, str)}
    a = up["ones_and_full_list"]
    assert {"entry_is_last_subtile", "leaves_at_last", "arrives_at_2_24", "stayed_inside", "two_risky_in_a_batch"} <= a["x"][0]
    assert a["y"][1] == list(range(PRE, PRE + MAXENT)) and "wild_fits" in a["y"][0] and "wild_misses" not in a["y"][0]
    b = up["first_term_and_overflow"]
    assert {"leaves_at_0", "arrives_at_2_24"} <= b["x"][0] and b["y"][1] == list(range(PRE, PRE + MAXENT + 1))
    c = up["even_index_tie_and_wild_miss"]
    assert {"leaves_at_even_index", "second_column_fails"} <= c["x"][0] and "wild_misses" in c["y"][0]
    d = up["wrong_table_binade_and_twice"]
    assert "table_key_is_not_the_accumulators" in d["x"][0] and "leaves_twice" in d["y"][0]
    # a list of zero or one entries: one record past the pre-chain's sub-tiles (and a last sub-tile of one particle)
    assert all(len(shapes[(1281, c)][ax][1]) <= 2 for c in fs.CLOUDS for ax in ("x", "y"))


# ---------------------------------------------------------------------------------------------------------------- GPU side
@pytest.mark.parametrize("N,cloud", UPDATE_CASES, ids=[f"{n}-{c}" for n, c in UPDATE_CASES])
def test_update_chains_match_the_oracle_riding_and_alone(update_sides, maps, gpu_ctx, N, cloud):
    m = maps[fs.MAP]
    p, poses, scans, res, after = update_sides[(N, cloud)]
    if cloud == "dominant":
        # (at 20 000 particles the others' floor weights add up to a sixth of the total: the one still outweighs them all together)
        w = after["weight"]
        assert w.max() > 0.5 and int(w.argmax()) == N // 2
    else:
        fs.check_intent(cloud, N, res, after)
    for riding in (True, False):
        g = bl.OccupancyGrid.from_cells(m["cells"], m["origin"], m["mpc"], cellsPerMeter=helpers.CPM_DEFAULT, ctx=gpu_ctx)
        gm = bl.OccupancyGrid.from_cells(m["cells"], m["origin"], m["mpc"], cellsPerMeter=helpers.CPM_DEFAULT, ctx=gpu_ctx)
        pf = bl.ParticleFilter(N, ctx=gpu_ctx)
        mapper = bl.Mapping(5.0, 4, 1, ctx=gpu_ctx)
        try:
            pf.setParticles(p)
            pf.debugEnable(True)
            pf.updateFilter(bl.make_pose(*poses[0], utime=scans[0].utime), scans[0], g, rand_value=777, want_pose=False)      # latches the odometry
            pf.setParticles(p)
            for k in (1, 2):
                r = res[k - 1]
                odo = bl.make_pose(*poses[k], utime=scans[k].utime)
                if riding:
                    assert pf.updateBegin(odo, scans[k], g, fs.RANDS[k - 1], noise=r["noise"])
                    mapper.updateMapFinishingFilter(scans[k], pf, scans[k].utime, gm)
                    pose = pf.poseEstimate()
                else:
                    pose = pf.updateFilter(odo, scans[k], g, rand_value=fs.RANDS[k - 1], noise=r["noise"])
                where = (N, cloud, "riding" if riding else "alone", k)
                stats = pf.debugEstimateStats()
                idx, like = pf.debugLast()
                assert np.array_equal(idx, r["idx"]), where                    # k = 2: drawn from the prefix update 1 left
                assert np.array_equal(like.astype(np.float64) * 0.5, r["raw"]), where
                assert fs._bits(pose) == fs._bits(r["pose"]), where + ((pose.x, pose.y, pose.theta), (r["pose"].x, r["pose"].y, r["pose"].theta), stats)
                print("estimate stats", where, stats)
                if k == 1:
                    got = pf.particles()
                    for f in ("x", "y", "theta"):
                        assert np.array_equal(got[f], after[f]), where + (f,)
                    assert np.allclose(got["weight"], after["weight"], rtol=1e-5, atol=0), where
        finally:
            mapper.close(); pf.close(); g.close(); gm.close()


@pytest.mark.parametrize("name", sorted(upload_sets()))
def test_built_chains_match_the_oracle(oracle, gpu_ctx, name):
    x, y = upload_sets()[name]
    p = np.zeros(UP_N, PARTICLE_DTYPE)
    p["x"], p["y"] = x, y
    pf = bl.ParticleFilter(UP_N, ctx=gpu_ctx)
    try:
        pf.setParticles(p, np.full(UP_N, 1000, np.uint32))
        est = pf.estimatePosteriorPose()
        stats = pf.debugEstimateStats()
        got = pf.particles()
        assert np.all(got["weight"] == 2.0 ** -13)
        want = oracle_lib.OPose()
        oracle.lib.orc_estimate_pose(np.ascontiguousarray(got).ctypes.data, UP_N, C.byref(want))
        # the oracle's loop is the census' loop
        for ax, v in (("x", x), ("y", y)):
            assert serial_sum(upload_terms(v))[-1].view(np.uint32) == np.float32(getattr(want, ax)).view(np.uint32), (name, ax)
        a = np.array([est.x, est.y], np.float32).view(np.uint32)
        b = np.array([want.x, want.y], np.float32).view(np.uint32)
        assert np.array_equal(a, b), (name, (est.x, est.y), (want.x, want.y), stats)
        print("estimate stats", name, stats)
        if name == "ones_and_full_list":
            # y: every one of the MAXENT listed sub-tiles went by its wild map, nothing was replayed or walked
            assert stats[4:] == [0, 0, MAXENT, 0], stats
        if name == "first_term_and_overflow":
            assert stats[6] == 0, stats                                      # y: no list (its counters stay where they were)
    finally:
        pf.close()
