"""The model of the range table (tests/range_table_model.py) against a plain-loop implementation with its own walk and square root, the
heading rule at its edges, the rules of the entries that the definition spells out, update against build, and the reason for the
feature: the scoring by table tells beam_cases.two_walls()'s poses apart as the exact cast does."""
import math

import numpy as np
import pytest

import beam_cases as bc
import beam_model as bm
import range_table_cases as rc
import range_table_model as rm

F32 = np.float32


def plain_table(cells, D, occ_min):
    """T by the reference's loop itself, cell by cell, with math.isqrt."""
    H, W = cells.shape
    out = np.full((H, W, len(D)), rm.NONE, np.uint16)
    for y0 in range(H):
        for x0 in range(W):
            for h, (ddx, ddy) in enumerate(D.tolist()):
                x1, y1 = x0 + ddx, y0 + ddy
                dx, dy = abs(ddx), abs(ddy)
                sx, sy = (1 if x0 < x1 else -1), (1 if y0 < y1 else -1)
                err, x, y = dx - dy, x0, y0
                while x != x1 or y != y1:
                    if 0 <= x < W and 0 <= y < H and cells[y, x] >= occ_min:
                        out[y0, x0, h] = math.isqrt(16 * ((x - x0) ** 2 + (y - y0) ** 2))
                        break
                    e2 = 2 * err
                    if e2 >= -dy:
                        err -= dy
                        x += sx
                    if e2 <= dx:
                        err += dx
                        y += sy
    return out


@pytest.mark.parametrize("case", [lambda: rc.single_cell(False, 1), lambda: rc.single_cell(True, 3), lambda: rc.strip(37, 1, 64, 3),
                                  lambda: rc.strip(1, 37, 64, 100), lambda: rc.room(23, 17, 64, 7), lambda: rc.room(23, 17, 128, 30, occ_min=2),
                                  lambda: rc.uniform(True), lambda: rc.uniform(False), lambda: rc.far_cell()])
def test_model_against_plain_loops(case):
    c = case()
    assert np.array_equal(c["table"], plain_table(c["cells"], c["D"], c["params"]["occ_min"]))


def test_directions_and_heading_limits():
    D = rm.directions(100, 256)
    assert D[0].tolist() == [100, 0] and D[64].tolist() == [0, 100] and D[128].tolist() == [-100, 0] and D[32].tolist() == [71, 71]
    assert np.abs(D).max() == 100 and np.array_equal(D[128:], -D[:128])
    for hn in (32, 63, 96, 2048, 0, -64):
        assert not rm.headings_ok(hn)
        with pytest.raises(rm.ArgError):
            rm.directions(10, hn)
    assert all(rm.headings_ok(hn) for hn in (64, 128, 256, 512, 1024))
    with pytest.raises(rm.ArgError):
        rm.check_entries(2 ** 25 + 1, 1, 64)
    rm.check_entries(2 ** 25, 1, 64)


@pytest.mark.parametrize("hn", [64, 128, 256, 512, 1024])
def test_heading_rule(hn):
    pi_f = F32(math.pi)
    assert rm.h_index([pi_f, -pi_f, np.nextafter(pi_f, F32(0)), -np.nextafter(pi_f, F32(0))], hn).tolist() == [hn // 2] * 4
    assert rm.h_index([0.0, -0.0], hn).tolist() == [0, 0]
    step = 2.0 * math.pi / hn
    assert rm.h_index([-step, -2 * step, -(hn // 4) * step], hn).tolist() == [hn - 1, hn - 2, 3 * hn // 4]       # negative a through the mask
    # products at exact .5: with kf a float, a = (j + 0.5) / kf need not give j + 0.5 back; take angles whose product is exactly that
    kf = rm.heading_scale(hn)
    exact = []
    for j in range(-hn // 2, hn // 2):
        a = F32((j + 0.5) / float(kf))
        for cand in (a, np.nextafter(a, F32(4)), np.nextafter(a, F32(-4))):
            if float(F32(cand * kf)) == j + 0.5:
                exact.append((cand, j))
                break
    assert len(exact) > hn // 4
    got = rm.h_index([e[0] for e in exact], hn)
    assert got.tolist() == [(e[1] + 1) & (hn - 1) for e in exact]             # floor(j + 0.5 + 0.5) = j + 1: a tie goes up
    # the floats either side of them and a sweep of the circle, against the rule one scalar operation at a time
    sweep = [np.nextafter(e[0], F32(s)) for e in exact for s in (-4, 4)] + np.linspace(-math.pi, math.pi, 4001).astype(np.float32).tolist()
    want = [int(math.floor(float(F32(F32(F32(a) * kf) + F32(0.5))))) & (hn - 1) for a in sweep]
    assert rm.h_index(sweep, hn).tolist() == want and set(want) == set(range(hn))


def test_occupied_start_and_far_cell():
    c = rc.room(23, 17, 64, 7)
    assert (c["table"][c["cells"] >= 1] == 0).all()
    rc.far_cell()                                                             # asserts k = K unseen and k = K - 1 seen
    assert int(rm.build(np.full((1, 1), -20, np.int8), rm.directions(4096, 64), 1).max()) == rm.NONE
    far = np.full((1, 1), 0, np.int64)
    assert int(bm.quarter(4095, 4095, far, far).max()) == 23164 < 23170 < rm.NONE


@pytest.mark.parametrize("edits", [[(11, 8, None)], [(0, 0, -20), (1, 0, -20), (0, 1, -20)], [(22, 16, -20), (21, 15, None)],
                                   [(5, 5, None), (17, 12, None), (9, 3, None)]])
def test_update_equals_build(edits):
    c = rc.room(23, 17, 64, 7)
    cells, box = rc.changed(c, edits)
    assert not np.array_equal(cells, c["cells"])
    fresh = rm.build(cells, c["D"], 1)
    got = rm.update(c["table"].copy(), cells, c["D"], 1, c["reach"], box)
    assert np.array_equal(got, fresh) and not np.array_equal(fresh, c["table"])
    for box0 in ((3, 3, 2, 5), (0, 4, 5, 3), (-9, -9, -1, -1), (23, 0, 30, 5), (0, 17, 5, 20)):
        t = c["table"].copy()
        assert rm.widened(box0, c["reach"], 23, 17) is None and np.array_equal(rm.update(t, cells, c["D"], 1, c["reach"], box0), c["table"])
    assert rm.widened((-50, -50, 50, 50), 7, 23, 17) == (0, 0, 22, 16)
    with pytest.raises(rm.ArgError):
        rm.update(c["table"].copy(), cells[:-1], c["D"], 1, c["reach"], box)


@pytest.mark.parametrize("hn", [64, 128, 256, 512])
def test_two_walls_told_apart_by_table(hn):
    """The reason for the beam model, kept by the table form: S(A) > S(B), and B sits at the floor unit for the default span."""
    c = rc.score_case(bc.two_walls(), hn)
    t = bm.make_tables(c["params"], c["cpm"])
    S = rm.scores(c["table"], c["origin"], c["cpm"], c["ranges"], c["thetas"], c["poses"], c["params"], t)
    exact = bm.scores(c["cells"], c["origin"], c["cpm"], c["ranges"], c["thetas"], c["poses"], c["params"], t)
    print("Hn", hn, "table S(A), S(B)", S.tolist(), "cast", exact.tolist())
    assert S[0] > S[1]
    assert bm.units(S, c["params"]["span"]).tolist() == [2 ** 20, 1]
    rays = bm.used_rays(c["ranges"], c["thetas"], c["params"])
    for i in range(2):
        g, e = rm.lookup(c["table"], c["origin"], c["cpm"], rays, c["poses"][i], c["params"], t), bm.cast(c["cells"], c["origin"], c["cpm"], rays, c["poses"][i], c["params"], t)
        assert np.abs(g["zstar"] - e["zstar"]).max() <= 1                     # quarter cells


def test_state_rules():
    p = bm.params(max_range=1.5, occ_min=1)
    rm.check_state(True, 1, 30, 20.0, p)
    for args in ((False, 1, 30, 20.0), (True, 2, 30, 20.0), (True, 1, 31, 20.0), (True, 1, 30, 10.0)):
        with pytest.raises(rm.StateError):
            rm.check_state(*args, p)
