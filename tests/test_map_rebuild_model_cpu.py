"""The map rebuild on the CPU (no GPU): the composition rule behind bl_scanlog_rebuild, the restated chunked fold against the sequential
oracle on every case of tests/map_rebuild_cases.py, and the proof that each case reaches its path (counts of chunks, pairs and
clamped cells, printed per case).  The saturation cases must tell the real rule from sum-then-clamp."""
import numpy as np
import pytest

import map_rebuild_cases as cases
import map_rebuild_model as mm

ODDS = [0, 1, 3, 4, 127]
STARTS = np.arange(-128, 128, dtype=np.int64)


def _fold(seq, hit, miss):
    f = mm.IDENTITY
    for H, M in seq:
        f = mm.f_scan(f, H, M, hit, miss)
    return f


def _random_seq(rng):
    n = int(rng.integers(1, 13))
    big = rng.random(n) < 0.3
    H = np.where(big, rng.integers(0, 8193, n), rng.integers(0, 4, n))
    M = np.where(rng.random(n) < 0.3, rng.integers(0, 8193, n), rng.integers(0, 4, n))
    H[rng.random(n) < 0.3] = 0
    M[rng.random(n) < 0.3] = 0
    return [(int(h), int(m)) for h, m in zip(H, M)]


def test_composition_identity_for_every_start_value_and_split():
    """Folding a sequence of scans into one (a, lo, hi) with `a` saturated to +-255, in two parts split anywhere and recombined, gives
    the sequential result for all 256 start values; the composed function fits (int16, int8, int8)."""
    rng = np.random.default_rng(7)
    differs = 0
    for _ in range(4000):
        hit, miss = int(rng.choice(ODDS)), int(rng.choice(ODDS))
        seq = _random_seq(rng)
        want = mm.sequential(STARTS, seq, hit, miss)
        differs += int((mm.sum_then_clamp(STARTS, seq, hit, miss) != want).any())
        for cut in range(len(seq) + 1):
            f1, f2 = _fold(seq[:cut], hit, miss), _fold(seq[cut:], hit, miss)
            for f in (f1, f2):
                assert -255 <= f[0] <= 255 and -128 <= f[1] <= f[2] <= 127
            assert np.array_equal(mm.f_apply(f2, mm.f_apply(f1, STARTS)), want), (hit, miss, seq, cut)
            assert np.array_equal(mm.f_apply(mm.f_then(f1, f2), STARTS), want), (hit, miss, seq, cut)
    print("sequences on which sum-then-clamp is wrong for some start value:", differs, "of 4000")
    assert differs > 1000


def test_composition_at_the_extremes():
    """Odds of 127 with 8192 rays in both passes, repeated and alternated: every add is far past the saturation of `a`."""
    for seq in ([(8192, 8192)] * 3, [(8192, 0), (0, 8192)] * 2, [(0, 8192), (8192, 0), (1, 0), (0, 1)], [(2, 0)] * 70 + [(0, 3)] * 90):
        for hit, miss in [(127, 127), (127, 1), (1, 127), (4, 1)]:
            want = mm.sequential(STARTS, seq, hit, miss)
            for cut in range(len(seq) + 1):
                got = mm.f_apply(_fold(seq[cut:], hit, miss), mm.f_apply(_fold(seq[:cut], hit, miss), STARTS))
                assert np.array_equal(got, want), (seq[:4], hit, miss, cut)


def test_walk_closed_form_equals_the_loop():
    """walk_cells (the closed form the kernels restate) against Mapping::bresenham's loop, transcribed."""
    def loop(x, y, x2, y2):
        dx, dy = abs(x2 - x), abs(y2 - y)
        sx, sy = (1 if x < x2 else -1), (1 if y < y2 else -1)
        err, out = dx - dy, []
        while x != x2 or y != y2:
            out.append((x, y))
            e2 = 2 * err
            if e2 >= -dy:
                err -= dy; x += sx
            if e2 <= dx:
                err += dx; y += sy
        return out

    rng = np.random.default_rng(3)
    ends = [(0, 0), (5, 0), (0, -5), (7, 7), (-7, 7), (64, 1), (1, -64), (130, 65), (-65, -130)] + [tuple(v) for v in rng.integers(-150, 151, (300, 2))]
    for ex, ey in ends:
        x, y = mm.walk_cells(3, -2, 3 + int(ex), -2 + int(ey))
        assert list(zip(x.tolist(), y.tolist())) == loop(3, -2, 3 + int(ex), -2 + int(ey)), (ex, ey)


@pytest.mark.parametrize("name", sorted(cases.BUILDERS))
def test_case_reaches_its_path_and_the_fold_equals_the_oracle(oracle, name):
    case = cases.get(name, oracle)
    res = cases.evaluate(case, oracle)                          # fold == truth, the condition, clamped > 0 where it must be
    assert res["truth"].shape == (case.height, case.width)


def test_saturation_cases_cannot_pass_on_sum_then_clamp(oracle):
    n = 0
    for name in sorted(cases.BUILDERS):
        case = cases.get(name, oracle)
        if case.saturates:
            res = cases.evaluate(case, oracle)
            assert res["clamped"] > 0 and not np.array_equal(res["naive"], res["truth"]), name
            n += 1
    assert n >= 15
