"""tests/adaptive_cases.py on the model alone: every case is what its name says -- the distinct-key counts, the k_sat and n(k)
values, which values clamp and which do not, which chain of commanded counts runs which (active, next) pairs, and that an update on
the all-free map leaves an all-floor record on the reference filter.  No GPU."""
import math

import numpy as np
import pytest

import adaptive_cases as ac
import adaptive_model as am
import oracle_lib
from botlab_amd.host import PARTICLE_DTYPE


def _k(case):
    p = case.params
    k = am.count_bins(case.x, case.y, case.th, p.bin_xy, p.bin_theta)
    assert k == len(ac.explicit_bins(case.x, case.y, case.th, p.bin_xy, p.bin_theta)), case.name      # the model against math.floor
    assert k == case.k, (case.name, k, case.k)                                                         # ... and what the builder states
    return k


def _keys(case):
    p = case.params
    return am.bin_keys(case.x, case.y, case.th, p.bin_xy, p.bin_theta)


def test_every_case_is_a_whole_cloud_inside_the_map():
    names = set()
    for c in ac.count_cases():
        assert 2 <= c.cap <= 8192 and c.x.size == c.cap and 2 <= c.params.min_particles <= c.cap, c.name
        assert np.all(np.isfinite(c.x)) and np.all(np.isfinite(c.y)) and np.all(np.isfinite(c.th)), c.name
        assert np.abs(c.x).max() < 3.5 and np.abs(c.y).max() < 3.5 and np.abs(c.th).max() <= ac.PI_F, c.name
        names.add(c.name)
        _k(c)
    assert len(names) == len(ac.count_cases())
    free = ac.free_map()
    assert free.shape == (200, 200) and np.all(free < 0)
    # the map spans [-5, 5): a pose within 3.5 m and a one-metre ray stay inside it
    assert ac.FREE_ORIGIN[0] + ac.FREE_SIDE * ac.FREE_MPC >= 4.99 and ac.short_scan(0)[0].max() <= 1.0


@pytest.mark.parametrize("cap", ac.SIZES)
def test_sizes(cap):
    own, one = ac.own_bin(cap), ac.one_bin(cap)
    assert own.cap == one.cap == cap
    assert _k(own) == cap and _k(one) == 1
    assert len(np.unique(np.stack([one.x, one.y, one.th]), axis=1).T) == cap          # distinct poses, one bin
    for c in (own, one):
        assert am.k_sat(cap, c.params.epsilon, c.params.z) == cap + 1                  # the count is exact: no k reaches the capacity
    # sizes on both sides of a wave, of a 256-thread workgroup and of its 1024 parents
    assert {63, 64, 65, 255, 256, 257, 1023, 1024, 1025} <= set(ac.SIZES) and max(ac.SIZES) > 4 * ac.WG


@pytest.mark.parametrize("bxy", [ac.BXY, 0.5])
def test_edges(bxy):
    c = ac.edges(bxy)
    e = ac.edge_values()
    n = e.size // 2
    # an edge and the float below it lie in different bins, whichever side of k * bin the float edge itself fell on
    on, below = e[:n].astype(float), e[n:].astype(float)
    assert np.all(below < on) and np.all(np.nextafter(e[n:], np.float32(np.inf)) == e[:n])
    if bxy == ac.BXY:
        ideal = np.arange(-20, 21)
        fl = np.array([math.floor(v / bxy) for v in on])
        assert set(fl - ideal) == {0, -1}                                              # some float edges are below k * 0.1 in double
        assert np.float32(0.3).astype(float) / 0.1 >= 3.0 and np.float32(0.7).astype(float) / 0.1 < 7.0
        assert math.floor(float(np.float32(-0.3)) / 0.1) == -4 and int(float(np.float32(-0.3)) / 0.1) == -3    # floor is not truncation
    k = _k(c)
    kx = len({math.floor(v / bxy) for v in e.astype(float)})
    # x edges (y, theta fixed), y edges, thetas: three families that share no key
    kth = len({math.floor(v / ac.BTH) for v in ac.THETA_EDGES.astype(float)})
    assert kth == 5                                                                    # +-pi, their neighbours, and +-0 in one bin
    assert math.floor(float(ac.PI_F) / ac.BTH) == 18 and math.floor(float(np.nextafter(ac.PI_F, np.float32(0))) / ac.BTH) == 17
    assert math.floor(float(-ac.PI_F) / ac.BTH) == -19 and math.floor(float(np.nextafter(-ac.PI_F, np.float32(0))) / ac.BTH) == -18
    # the x family and the y family share exactly the pose bin of (0.05, 0.05, 0.05), once each
    assert k == 2 * kx - 1 + kth
    assert np.signbit(c.th[-1]) and c.th[-1] == 0.0 and not np.signbit(c.th[-2])


def test_clamps():
    c = ac.clamps()
    L = ac.LIM
    n = len(ac.CLAMP_Q)
    for q in ac.CLAMP_Q:
        v = float(ac.clamp_value(q))
        assert math.floor(v / ac.CLAMP_BIN) == q, q                                    # the float lies in the bin it is named for
        assert abs(v) < 1.06
    idx = am.bin_index(np.array([ac.clamp_value(q) for q in ac.CLAMP_Q]), ac.CLAMP_BIN) - L
    assert list(idx) == [L - 2, L - 1, L - 1, L - 1, L - 1, -L + 1, -L, -L, -L, -L]    # inside stays; on and beyond share the end bin
    keys = _keys(c)
    for axis in range(3):
        sl = keys[axis * n:(axis + 1) * n]
        assert len(set(sl[1:5])) == 1 and sl[0] != sl[1] and len(set(sl[6:10])) == 1 and sl[5] != sl[6]
        assert len(set(sl)) == 4
    assert _k(c) == 12
    assert am.k_sat(c.cap, c.params.epsilon, c.params.z) == c.cap + 1


def test_dedup_levels():
    want = {"dedup_same_in_each_wg": 1024, "dedup_equal_per_wg": 4, "dedup_one_common": 1 + 4 * 1023, "dedup_only_x": 4096,
            "dedup_only_y": 4096, "dedup_only_t": 4096}
    cases = {c.name: c for c in ac.dedup_cases()}
    assert set(cases) == set(want)
    for name, c in cases.items():
        assert c.cap == 4 * ac.WG and _k(c) == want[name], name
        assert am.k_sat(c.cap, c.params.epsilon, c.params.z) == c.cap + 1
    per_wg = lambda c: _keys(c).reshape(4, ac.WG)
    same = per_wg(cases["dedup_same_in_each_wg"])
    assert all(len(set(w)) == ac.WG for w in same) and all(np.array_equal(np.sort(same[0]), np.sort(w)) for w in same)
    eq = per_wg(cases["dedup_equal_per_wg"])
    assert all(len(set(w)) == 1 for w in eq) and len({w[0] for w in eq}) == 4
    com = per_wg(cases["dedup_one_common"])
    shared = set(com[0]) & set(com[1]) & set(com[2]) & set(com[3])
    assert len(shared) == 1 and all(len(set(w)) == ac.WG for w in com)                 # all distinct inside a workgroup: the LDS table half full
    assert all(len(set(com[a]) & set(com[b])) == 1 for a in range(4) for b in range(a))
    assert len({int(np.flatnonzero(w == next(iter(shared)))[0]) for w in com}) == 4    # at another slot in every workgroup
    for axis, name in enumerate(("dedup_only_x", "dedup_only_y", "dedup_only_t")):
        keys = _keys(cases[name])
        fields = np.stack([keys >> 42, (keys >> 21) & 0x1FFFFF, keys & 0x1FFFFF])
        for a in range(3):
            assert len(set(fields[a])) == (4096 if a == axis else 1), (name, a)
        other = [a for a in range(3) if a != axis]
        assert all(fields[a][0] >= ac.LIM for a in other)                              # the fixed fields are positive: their top bit is set


def test_ksat_setups():
    assert am.k_sat(1500, 0.3, ac.Z) == 805 and am.bound(804, 0.3, ac.Z) == 1499 and am.bound(805, 0.3, ac.Z) == 1501
    assert am.k_sat(2048, 0.2, ac.Z) == 729
    cases = {c.name: c for c in ac.ksat_cases()}
    assert len(cases) == 6
    for cap, eps, ks in ac.KSAT_SETUPS:
        assert am.k_sat(cap, eps, ac.Z) == ks and ac.WG < cap <= 2 * ac.WG            # two workgroups
        for d in (ks - 1, ks, cap):
            c = cases[f"ksat_{cap}_{d}"]
            assert _k(c) == d and c.params.epsilon == eps
            assert len(set(_keys(c)[:ac.WG])) == min(d, ac.WG)                        # what the first workgroup alone holds
            m = am.CountModel(cap, c.params)
            m.counted(c.x, c.y, c.th)
            assert m.ksat == ks and m.bins == min(d, ks)
            if d < ks:
                assert m.bins == d and c.params.min_particles <= m.next < cap
            else:
                assert m.next == cap


def test_chains_run_the_pairs():
    for name, (cap, targets) in {**ac.CHAINS, **ac.PARITY_CHAINS}.items():
        assert cap <= 8192 and all(t is None or 2 <= t <= cap for t in targets)
        pairs = ac.chain_pairs(cap, targets)
        need = ac.REQUIRED_PAIRS.get(name) or ac.PARITY_PAIRS[name]
        assert set(need) <= set(pairs), (name, set(need) - set(pairs))
        assert all(a != b for a, b in need)                                           # every required pair shrinks or grows
    seen = {p for name, (cap, t) in ac.CHAINS.items() for p in ac.chain_pairs(cap, t)}
    # the issue's list: two records, a wave +- 1, a strict chunk (128) +- 1, MCL_BLOCK = SCAN_TILE = 512 +- 1, STRICT_PAR_MIN = 4096 +- 1
    for p in [(4096, 2), (2, 4096), (4096, 63), (4096, 64), (4096, 65), (65, 64), (64, 65), (127, 128), (128, 129), (511, 512), (512, 513),
              (8192, 4095), (8192, 4096), (8192, 4097), (4095, 8192), (4096, 8192), (4097, 8192)]:
        assert p in seen, p
    # a cloud inside the one bin of ONE_BIN counts k = 1, and k = 1 commands min_particles
    p = ac.track_cloud(4096, PARTICLE_DTYPE, 0)
    assert am.count_bins(p["x"], p["y"], p["theta"], ac.ONE_BIN["binXY"], ac.ONE_BIN["binTheta"]) == 1
    for t in (2, 63, 4097):
        assert am.next_count(1, t, ac.ONE_BIN["epsilon"], ac.Z, 8192) == t


def test_all_floor_record_on_the_reference(oracle):
    """An update on the all-free map: every raw likelihood of the reference is at or below the floor (0.001), so its
    computeNormalizedPosterior leaves FLOOR_ACTIVE equal weights -- the serial sum's 0.001 / (0.001 + ... + 0.001), not 1 / n."""
    n = ac.FLOOR_ACTIVE
    assert n != ac.FLOOR_CAP and ac.FLOOR_NEXT not in (n, ac.FLOOR_CAP)
    opf = oracle_lib.OraclePF(oracle, n)
    opf.set_particles(ac.track_cloud(n, PARTICLE_DTYPE, 1000))
    res = ac.floor_update(oracle, opf)
    assert np.all(res["raw"] <= 0.001) and np.array_equal(res["idx"], np.arange(n))
    w = opf.particles()["weight"]
    assert len(set(w)) == 1 and w[0] == ac.serial_floor_weight(n)
    assert w[0] != ac.serial_floor_weight(ac.FLOOR_CAP) and w[0] != 1.0 / n          # neither the capacity's floor weight nor 1 / n
    assert ac.serial_floor_weight(ac.FLOOR_NEXT) != 1.0 / ac.FLOOR_NEXT
