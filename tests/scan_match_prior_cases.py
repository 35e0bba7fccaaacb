"""Inputs for the scan match with a prior (bl_scanmatch_match_prior) and the proof -- on the CPU, from the model
(tests/scan_match_prior_model.py) alone -- that each one reaches the condition it is named for.  Shared by
tests/test_scan_match_prior_model_cpu.py and tests/test_gpu_scan_match_prior.py; everything is built here in code.

A builder returns a PCase; evaluate(case) runs the model once (cached) and asserts the case's property."""
import math
from collections import namedtuple

import numpy as np

import helpers
import scan_match_cases as smc
import scan_match_model as sm
import scan_match_prior_model as smp

F32 = np.float32
CPM = helpers.CPM_DEFAULT
MPC = F32(0.05)
DTH = smc.DTH
DEG1 = smc.DEG1
UTIME = 4321
MID_HALF_LIFE = 777                     # not a power of two: the quotient and the remainder of d / half_life both vary

PCase = namedtuple("PCase", "name cells origin mpc cpm ranges thetas centre window dtheta max_range min_score prior half_life prop")


def make(name, cells, ranges, thetas, centre, window, prior, half_life, prop, origin=(0.0, 0.0), dtheta=DTH, max_range=8.0, min_score=0):
    assert smp.check_prior(*prior, half_life=half_life, want_moments=half_life is not None), (name, prior, half_life)
    return PCase(name, np.ascontiguousarray(cells, dtype=np.int8), (float(origin[0]), float(origin[1])), MPC, F32(CPM),
                 np.asarray(ranges, dtype=np.float32), np.asarray(thetas, dtype=np.float32), tuple(F32(v) for v in centre),
                 tuple(int(v) for v in window), F32(dtheta), float(max_range), int(min_score), tuple(int(v) for v in prior),
                 half_life, prop)


def model(case, prior=None, half_life="case"):
    nx, ny, nt = case.window
    return smp.match(case.cells, case.origin, case.mpc, case.cpm, case.ranges, case.thetas, case.centre, nx, ny, nt, case.dtheta,
                     case.max_range, prior=case.prior if prior is None else prior,
                     half_life=case.half_life if half_life == "case" else half_life, min_score=case.min_score, utime=UTIME)


_evaluated = {}


def evaluate(case):
    if case.name not in _evaluated:
        ref = model(case)
        if case.prop is not None:
            case.prop(case, ref)
        if case.half_life is not None:
            for num, den in ref["fractions"]:
                assert den >= 1 and 2 * abs(num) <= den, (case.name, ref["fractions"])
        _evaluated[case.name] = ref
    return _evaluated[case.name]


def winner(ref):
    return ref["di"], ref["dj"], ref["dk"]


def tie_set(case, ref):
    nx, ny, nt = case.window
    ks, js, is_ = np.nonzero(ref["volume"] == ref["best_obj"])
    return [(i - nx, j - ny, k - nt) for k, j, i in zip(ks.tolist(), js.tolist(), is_.tolist())]


# ---------------------------------------------------------------------------------------------------------------- windows
ROOM_PRIOR = (300, 120, 400, 50)
WINDOWS = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (4, 4, 12), (64, 64, 2), (1, 1, 180)]


def window_name(w):
    return "window_%d_%d_%d" % w


def room_window(w):
    """The room of scan_match_cases (walls, three boxes, mixed log-odds) seen from a pose a little off the centre."""
    r, t = smc.room_scan(0.3)
    nx, ny, nt = w

    def prop(case, ref):
        ncand = (2 * nx + 1) * (2 * ny + 1)
        assert ref["rays_used"] == 72 and ref["score_volume"].max() > 0
        if w == (4, 4, 12):
            assert ncand % 64 != 0 and ((2 * nt + 1) * ncand) % 64 != 0
        if w == (64, 64, 2):
            threads, slices, per = smc.narrow_launch(w)
            assert threads == 1024 and slices > 1 and per % (2 * nx + 1) != 0           # a slice boundary inside a row
            assert 2 * nx + 1 == 129                                                     # three chunks of a moments row, the last one lane
    # max_range 9: a 64-cell shift slides max-range returns over the walls as well
    return make(window_name(w), smc.room(), r, t, (smc.ROOM_POSE[0] + 0.06, smc.ROOM_POSE[1] - 0.04, 0.3 + 0.01), w, ROOM_PRIOR,
                MID_HALF_LIFE, prop, max_range=9.0)


def width_203():
    """A grid whose width is no multiple of four: the byte-wise staging of the map window."""
    cells = smc.sparse_grid(150, 203, 77)
    r, t = smc.random_rays(100, 78, 0.2, 3.0)

    def prop(case, ref):
        assert case.cells.shape[1] == 203 and case.cells.shape[1] & 3
        assert smc.narrow_lds_request(float(case.ranges.max()), CPM, 9, 6, 203, 150) <= smc.SM_LDS_MAX   # staged: path 0
        assert ref["score"] > 0
    return make("width_203", cells, r, t, (5.0125, 3.7625, -0.7), (9, 6, 7), ROOM_PRIOR, MID_HALF_LIFE, prop)


def direct_path():
    """A long-range scan on a large grid: the endpoints span more cells than LDS holds and the grid is read directly (path 1),
    the way tests/test_gpu_scan_match.py reaches it."""
    cells = smc.sparse_grid(1200, 1200, 79)
    rays = 290
    thetas = (2.0 * np.pi * np.arange(rays) / rays).astype(np.float32)
    ranges = np.random.default_rng(80).uniform(0.2, 28.0, rays).astype(np.float32)

    def prop(case, ref):
        assert smc.narrow_lds_request(float(case.ranges.max()), CPM, 6, 4, 1200, 1200) > smc.SM_LDS_MAX
        assert ref["score"] > 0
    return make("direct_path", cells, ranges, thetas, (30.0125, 30.0125, 0.9), (6, 4, 3), ROOM_PRIOR, MID_HALF_LIFE, prop, max_range=50.0)


# ---------------------------------------------------------------------------------------------------------------- half lives
def half_life_case(hl):
    base = room_window((4, 4, 12))

    def prop(case, ref):
        nx, ny, nt = case.window
        w = smp.weights(ref["volume"], ref["best_obj"], hl)
        d = ref["best_obj"] - ref["volume"].astype(np.int64)
        assert int(w.max()) == 1 << 20
        if hl == 1:
            assert (d >= 21).any() and (w == 0).sum() > 0.9 * w.size                     # e >= 21 reached, nearly every weight 0
        elif hl == smp.MAX_HALF_LIFE:
            assert int(w.min()) > 1 << 19 and d.max() > 0                                # every weight near 2^20: the largest sums
        else:
            assert (w == 0).sum() < w.size // 2 and len(np.unique(w)) > 64
    return base._replace(name="half_life_%d" % hl, half_life=hl, prop=prop)


def negative_axy():
    base = room_window((4, 4, 12))

    def prop(case, ref):
        assert case.prior[1] < 0
        nx, ny, nt = case.window
        p = smp.pen_volume(case.prior, nx, ny, nt)
        assert p[nt, ny + 3, nx + 3] < p[nt, ny + 3, nx - 3]                             # the cross term shows
    return base._replace(name="negative_axy", prior=(300, -200, 400, 50), prop=prop)


# ---------------------------------------------------------------------------------------------------------------- the prior decides
def prior_moves_winner():
    """One ray, two occupied cells: 100 at di = 3, 60 at di = 1.  The prior takes 52 off the first and 5 off the second: the winner
    is not the raw-score maximum."""
    def prop(case, ref):
        raw = ref["raw_best"]
        assert raw[:3] == (3, 0, 0) and raw[3] == 100
        assert winner(ref) == (1, 0, 0) and ref["score"] == 60 and ref["best_obj"] == 55 and ref["pen_best"] == 5 and ref["ties"] == 1
        assert ref["score"] < raw[3]
    case = make("prior_moves_winner", smc.free_map(40, 60, [(33, 20), (31, 20)]), *smc.ONE_RAY, smc.ONE_CENTRE, (4, 3, 1),
                (1500, 0, 0, 256), MID_HALF_LIFE, prop)          # a_tt: a heading step costs one unit
    case.cells[20, 31] = 60
    return case


def corridor_cells():
    cells = np.full((64, 64), -100, np.int8)
    cells[22, :] = 100
    cells[42, :] = 100
    return cells


def corridor_rays():
    """From cell (32.5, 32.5), heading 0, rays onto the two walls only (10 cells away): the corridor's ends are never seen."""
    angles = np.concatenate([np.radians(np.arange(40.0, 141.0, 4.0)), -np.radians(np.arange(40.0, 141.0, 4.0))])
    ranges = (10.0 * 0.05) / np.abs(np.sin(angles))
    return ranges.astype(np.float32), angles.astype(np.float32)


CORRIDOR_CENTRE = (32.5 * 0.05, 32.5 * 0.05 + 0.05, 0.0)              # one cell off across the corridor


def corridor(prior, name):
    r, t = corridor_rays()

    def prop(case, ref):
        nx, ny, nt = case.window
        t_ = tie_set(case, ref)
        if case.prior == (0, 0, 0, 0):
            assert ref["ties"] > 1 and ref["score"] > 0
            same = [c for c in t_ if c[1:] == winner(ref)[1:]]
            assert len({c[0] for c in same}) == 2 * nx + 1, t_                          # flat along the corridor: every di ties
        else:
            assert case.prior[0] > 0 and ref["ties"] == 1 and len(t_) == 1
            free = evaluate(corridor((0, 0, 0, 0), "corridor_free"))
            assert winner(ref)[0] == 0 and all(abs(c[0]) >= abs(winner(ref)[0]) for c in tie_set(case, free))
            assert ref["score"] == free["score"]                                         # the prior chose among the raw maxima
    return make(name, corridor_cells(), r, t, CORRIDOR_CENTRE, (4, 4, 2), prior, MID_HALF_LIFE, prop, dtheta=DEG1)


def corridor_free():
    return corridor((0, 0, 0, 0), "corridor_free")


def corridor_prior():
    return corridor((300, 0, 0, 300), "corridor_prior")                  # a cell along the corridor, a heading step: one unit


# ---------------------------------------------------------------------------------------------------------------- flat maps
def flat_map(value, name):
    """Empty (0) or all-free (-127) map: obj = -pen, the centre wins by the key alone, the moments are those of -pen."""
    r, t = smc.room_scan(0.0)

    def prop(case, ref):
        nx, ny, nt = case.window
        assert int(ref["score_volume"].max()) == 0
        assert winner(ref) == (0, 0, 0) and ref["score"] == 0 and ref["best_obj"] == 0 and ref["pen_best"] == 0
        assert np.array_equal(ref["volume"].astype(np.int64), -smp.pen_volume(case.prior, nx, ny, nt))
        assert ref["ties"] == int((smp.pen_volume(case.prior, nx, ny, nt) == 0).sum()) > 1  # small shifts cost less than one unit
        assert ref["sums"] == smp.moment_sums(-smp.pen_volume(case.prior, nx, ny, nt), 0, case.half_life, nx, ny, nt)
    return make(name, np.full((64, 64), value, np.int8), r, t, (smc.ROOM_POSE[0], smc.ROOM_POSE[1], 0.0), (5, 4, 3), (90, 30, 70, 300), 3, prop)


# ---------------------------------------------------------------------------------------------------------------- window faces
def face(axis, sign):
    """The best candidate on one face of the window: its fraction along that axis is (0, 1), the others come from neighbours."""
    name = "face_%s_%s" % ("xyt"[axis], "plus" if sign > 0 else "minus")
    if axis < 2:
        n = 3
        cell = (30 + sign * n, 20) if axis == 0 else (30, 20 + sign * n)
        want = (sign * n, 0, 0) if axis == 0 else (0, sign * n, 0)
        # neighbours worth less than the cell itself: the winner's other axes have a real parabola
        cells = smc.free_map(40, 60, [cell])
        if axis == 0:
            cells[cell[1] + 1, cell[0]] = 40
            cells[cell[1] - 1, cell[0]] = 10
        else:
            cells[cell[1], cell[0] + 1] = 40
            cells[cell[1], cell[0] - 1] = 10
        rays, centre, window, dth = smc.ONE_RAY, smc.ONE_CENTRE, (n, n, 0), DTH
        prior = (0, 0, 0, 0)
    else:
        e = smc.long_ray_ends(2, DEG1)
        assert len(set(e.values())) == 5
        cells = smc.free_map(60, 120, [e[2 * sign]])
        want = (0, 0, 2 * sign)
        rays, centre, window, dth = smc.LONG_RAY, smc.ONE_CENTRE, (1, 1, 2), DEG1
        prior = (256, 0, 256, 0)                                                     # a shift costs a unit, a heading step nothing

    def prop(case, ref):
        assert winner(ref) == want and ref["ties"] == 1 and ref["score"] == 100, (winner(ref), want, ref["ties"])
        assert abs(want[axis]) == case.window[axis]
        assert ref["fractions"][axis] == (0, 1)
        if axis < 2:
            other = 1 - axis
            assert ref["fractions"][other] == (30, 2 * (200 - 50)) and ref["fractions"][2] == (0, 1)     # ntheta = 0
    return make(name, cells, *rays, centre, window, prior, MID_HALF_LIFE, prop, dtheta=dth)


def nx_zero():
    base = room_window((0, 3, 2))

    def prop(case, ref):
        assert ref["fractions"][0] == (0, 1)
    return base._replace(name="nx_zero", prop=prop)


# ---------------------------------------------------------------------------------------------------------------- the list
BUILDERS = {window_name(w): (lambda w=w: room_window(w)) for w in WINDOWS}
BUILDERS.update(width_203=width_203, direct_path=direct_path, negative_axy=negative_axy, prior_moves_winner=prior_moves_winner,
                corridor_free=corridor_free, corridor_prior=corridor_prior, nx_zero=nx_zero,
                flat_empty=lambda: flat_map(0, "flat_empty"), flat_free=lambda: flat_map(-127, "flat_free"))
for _hl in (1, MID_HALF_LIFE, smp.MAX_HALF_LIFE):
    BUILDERS["half_life_%d" % _hl] = (lambda hl=_hl: half_life_case(hl))
for _axis in range(3):
    for _sign in (-1, 1):
        BUILDERS["face_%s_%s" % ("xyt"[_axis], "plus" if _sign > 0 else "minus")] = (lambda a=_axis, s=_sign: face(a, s))

_cases = {}


def get(name):
    if name not in _cases:
        _cases[name] = BUILDERS[name]()
        assert _cases[name].name == name, (_cases[name].name, name)
    return _cases[name]
