"""bl_mapray_dev.h compiled for the host (tests/cpp/mapray_ref.cpp), without a GPU: the one copy of the map updates' ray geometry
and Bresenham walk that k_map_update, k_rb_map, k_rl_rays / k_rl_fold and k_obs_rays share.

  * the walk from k0 = 0 against the reference loop (mapping_cases.walk: Mapping::bresenham, mapping.cpp:101-127): every dx, dy <= 64
    in all four quadrants; dmaj on both sides of 32768 -- where the start's division goes from 32 to 64 bits -- with dmin 0, 1, 2,
    dmaj / 2, dmaj - 1, dmaj; and 16 steps from starts k0 > 0, which must be the same cells of the full walk;
  * the walk at the limit of traced rays, dmaj = 2^25 - 1 between coordinates +-(2^24 - 1): 64 steps from several k0 against the
    closed form in Python integers (the int carry of rem and the 64-bit start must survive it);
  * bl_walk_cell(ray, k) is the walker's cell k;
  * bl_ray_cells is rb_slam_model.ray_cells -- the oracle's moving scan truncated as mapping.cpp does -- on every update of every
    case of tests/mapping_cases.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mapping_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUADRANTS = ((1, 1), (-1, -1), (1, -1), (-1, 1))
LONG_DMAJ = (32767, 32768, 32769, 40000)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("mapray") / "mapray_ref.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "mapray_ref.cpp")])
    lib = C.CDLL(so)
    lib.mr_ray_cells.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def header_walk(ref, ray, k0, count):
    """Cells k0 .. k0 + count - 1 (as far as the walk goes) by the header's walker, as a list of (x, y)."""
    r = np.asarray(ray, np.int32)
    xy = np.zeros((max(count, 1), 2), np.int32)
    n = ref.mr_walk(_p(r), int(k0), int(count), _p(xy))
    return [tuple(c) for c in xy[:n].tolist()]


def closed_form(ray, k):
    """Cell k of the walk in Python integers: the major axis advances k, the minor axis floor((2 k dmin + dmaj) / (2 dmaj))."""
    x0, y0, x1, y1 = ray
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    sx, sy = (1 if x0 < x1 else -1), (1 if y0 < y1 else -1)
    if dx >= dy:
        return (x0 + sx * k, y0 + sy * ((2 * k * dy + dx) // (2 * dx)))
    return (x0 + sx * ((2 * k * dx + dy) // (2 * dy)), y0 + sy * k)


def _rays(dmaj, dmins, origin=(5, 7)):
    """(x0, y0, x1, y1) with (|dx|, |dy|) = (dmaj, dmin) and (dmin, dmaj) in all four quadrants."""
    for dmin in dmins:
        for a, b in {(dmaj, dmin), (dmin, dmaj)}:
            for qx, qy in QUADRANTS:
                yield (origin[0], origin[1], origin[0] + qx * a, origin[1] + qy * b)


def _long_dmins(dmaj):
    return sorted({0, 1, 2, dmaj // 2, dmaj - 1, dmaj})


def test_walk_is_the_reference_loop_for_short_rays(ref):
    for dx in range(65):
        for dy in range(65):
            for qx, qy in QUADRANTS:
                ray = (5, 7, 5 + qx * dx, 7 + qy * dy)
                want = mc.walk(*ray)
                assert ref.mr_ray_steps(_p(np.asarray(ray, np.int32))) == len(want) == max(dx, dy)
                assert header_walk(ref, ray, 0, len(want) + 3) == want, ray


_full = {}


def _full_walk(ray):
    if ray not in _full:
        _full[ray] = mc.walk(*ray)
    return _full[ray]


@pytest.mark.parametrize("dmaj", LONG_DMAJ)
def test_walk_is_the_reference_loop_across_the_division_width(ref, dmaj):
    for ray in _rays(dmaj, _long_dmins(dmaj)):
        want = _full_walk(ray)
        assert len(want) == dmaj
        assert header_walk(ref, ray, 0, dmaj) == want, ray


@pytest.mark.parametrize("dmaj", LONG_DMAJ)
def test_walk_from_a_later_start_is_the_same_cells(ref, dmaj):
    for ray in _rays(dmaj, _long_dmins(dmaj)):
        want = _full_walk(ray)
        for k0 in (1, 15, 16, 17, dmaj // 2, dmaj - 16, dmaj - 1):
            assert header_walk(ref, ray, k0, 16) == want[k0:k0 + 16], (ray, k0)


def test_walk_at_the_cell_limit(ref):
    lim = (1 << 24) - 1
    # coordinates +-(2^24 - 1), the outermost a traced ray has, span 2^25 - 2; dmaj = 2^25 - 1 itself starts one cell further out
    for span, lo in ((2 * lim, -lim), (2 * lim + 1, -lim - 1)):
        for dmin in (0, 1, span // 2, span - 1, span):
            for qx, qy in QUADRANTS:
                for xmajor in (True, False):
                    a0, a1 = (lo, lo + span) if qx > 0 else (lo + span, lo)
                    m = dmin if qy > 0 else -dmin
                    b0 = -(m // 2)
                    ray = (a0, b0, a1, b0 + m) if xmajor else (b0, a0, b0 + m, a1)
                    for k0 in (0, 1, 16, 32767, 32768, span // 2, span - 65, span - 64):
                        got = header_walk(ref, ray, k0, 64)
                        assert got == [closed_form(ray, k) for k in range(k0, k0 + 64)], (ray, k0)
                    assert header_walk(ref, ray, span - 3, 64) == [closed_form(ray, k) for k in range(span - 3, span)]


def test_walk_cell_is_the_walkers_cell(ref):
    rays = [(5, 7, 5 + qx * dx, 7 + qy * dy) for dx in (0, 1, 7, 64) for dy in (0, 1, 7, 64) for qx, qy in QUADRANTS if max(dx, dy) > 0]
    for dmaj in LONG_DMAJ:
        rays += list(_rays(dmaj, _long_dmins(dmaj)))
    lim = (1 << 24) - 1
    rays += [(-lim - 1, -3, lim, 5), (lim, lim, -lim - 1, -lim - 1), (4, lim, 3, -lim - 1)]
    for ray in rays:
        K = max(abs(ray[2] - ray[0]), abs(ray[3] - ray[1]))
        ks = np.unique(np.clip(np.array([0, 1, 15, 16, 17, 63, 64, K // 2, K - 17, K - 16, K - 2, K - 1]), 0, K - 1)).astype(np.int32)
        xy = np.zeros((len(ks), 2), np.int32)
        ref.mr_walk_cells(_p(np.asarray(ray, np.int32)), _p(ks), len(ks), _p(xy))
        for k, c in zip(ks.tolist(), xy.tolist()):
            assert [tuple(c)] == header_walk(ref, ray, k, 1) and tuple(c) == closed_form(ray, k), (ray, k)


def header_ray_cells(ref, case, scan, begin, end):
    """bl_ray_cells on the rays the host keeps (range > 0.15f), the rays that take no part left out: (n, 4) int64."""
    keep = scan.ranges > mc.MIN_RANGE
    ranges, thetas, times = (np.ascontiguousarray(a[keep]) for a in (scan.ranges, scan.thetas, scan.times))
    frame = np.array([case.origin[0], case.origin[1], case.mpc, case.cpm], np.float32)
    pb, pe = (np.array([p.x, p.y, p.theta], np.float32) for p in (begin, end))
    out = np.zeros((len(ranges), 4), np.int32)
    ref.mr_ray_cells(case.width, case.height, _p(frame), C.c_float(case.max_laser), _p(pb), int(begin.utime), _p(pe), int(end.utime), len(ranges),
                     _p(ranges), _p(thetas), _p(times), _p(out))
    return out[out[:, 0] != ref.mr_no_ray()].astype(np.int64)


@pytest.mark.parametrize("name", list(mc.BUILDERS))
def test_ray_cells_are_the_oracles(ref, oracle, name):
    case = mc.get(name, oracle)
    _, geo = mc.evaluate(case, oracle)
    prev, traced = None, 0
    for (scan, p), g in zip(case.updates, geo):
        pose = oracle.pose(p[0], p[1], p[2], utime=p[3])
        if prev is not None:
            got = header_ray_cells(ref, case, scan, prev, pose)
            assert np.array_equal(got, g["cells"]), name
            traced += len(got)
        prev = pose
    assert traced > 0 or name == "all_beyond_max"
