"""tests/scan_match_cases.py on the CPU: every case reaches what it is named for (evaluate asserts the property from the model),
and the tie constructions of group A really tell the levels of the candidate order apart: for each level there is a case on which
an order with that level reversed, or swapped with its neighbour, elects another candidate than the definition's."""
import numpy as np
import pytest

import scan_match_cases as smc
import scan_match_model as sm

LEVELS = ("d2", "adk", "dk", "dj", "di")


def levels(c):
    di, dj, dk = c
    return [di * di + dj * dj, abs(dk), dk, dj, di]


def elect(case, ev, key):
    """The candidate with the smallest key among those sharing the best score."""
    return min(smc.tie_set(case, ev), key=key)


def true_order(c):
    return tuple(levels(c))


def reversed_at(level):
    def key(c):
        v = levels(c)
        v[level] = -v[level]
        return tuple(v)
    return key


def swapped_at(level):
    def key(c):
        v = levels(c)
        v[level], v[level + 1] = v[level + 1], v[level]
        return tuple(v)
    return key


@pytest.mark.parametrize("name", list(smc.BUILDERS))
def test_case_reaches_what_it_claims(name):
    case = smc.get(name)
    ev = smc.evaluate(case)
    assert ev["ref"]["rays_used"] == len(sm.valid_rays(case.ranges, case.thetas, case.max_range)[0])
    if smc.is_narrow(case):
        nx, ny, nt = case.window
        assert ev["volume"].shape == (2 * nt + 1, 2 * ny + 1, 2 * nx + 1)
        assert sm.best_candidate(ev["volume"], nx, ny, nt)[:3] == smc.winner(ev)


def test_every_case_of_group_a_ties_at_a_positive_score():
    for name in smc.GROUP_A:
        case = smc.get(name)
        ev = smc.evaluate(case)
        assert ev["ref"]["score"] > 0 and ev["ref"]["ties"] >= 2, name
        assert elect(case, ev, true_order) == smc.winner(ev), name           # the order spelled here is the model's


# the case that tells each mutation from the definition
REVERSED = {"d2": "a_d2", "adk": "a_three_headings", "dk": "a_dk_pm1", "dj": "a_dj_before_di", "di": "a_di"}
REVERSED_FAR = {"dk": "a_dk_sign", "di": "a_di_sign"}                        # |dk|, |di| >= 2: the sign bit alone
SWAPPED = {"d2": "a_headings_and_shifts", "adk": "a_three_headings", "dj": "a_cross"}   # level <-> the next one


@pytest.mark.parametrize("level", range(5))
def test_a_reversed_level_elects_another_candidate(level):
    for table in (REVERSED, REVERSED_FAR):
        name = table.get(LEVELS[level])
        if name is None:
            continue
        case = smc.get(name)
        ev = smc.evaluate(case)
        assert elect(case, ev, reversed_at(level)) != smc.winner(ev), (LEVELS[level], name)
        for other in range(level):                                           # and it is this level that decides: the ones above tie
            assert len({levels(c)[other] for c in (elect(case, ev, reversed_at(level)), smc.winner(ev))}) == 1, (name, other)


@pytest.mark.parametrize("level", [0, 1, 3])
def test_a_level_swapped_with_the_next_elects_another_candidate(level):
    case = smc.get(SWAPPED[LEVELS[level]])
    ev = smc.evaluate(case)
    assert elect(case, ev, swapped_at(level)) != smc.winner(ev), LEVELS[level]


def test_sign_bits_decide_alone():
    for name, field in (("a_di_sign", 0), ("a_dk_sign", 2)):
        case = smc.get(name)
        ev = smc.evaluate(case)
        a, b = smc.tie_set(case, ev)
        assert a[field] == -b[field] and abs(a[field]) >= 2 and all(a[f] == b[f] for f in range(3) if f != field), (a, b)


def test_group_h_sits_either_side_of_the_limit():
    under = smc.narrow_lds_request(9.64, smc.CPM, 0, 0, 1000, 1000)
    over = smc.narrow_lds_request(9.66, smc.CPM, 0, 0, 1000, 1000)
    assert under <= smc.SM_LDS_MAX < over, (under, over)
    assert [((w + 3) & ~3) * h for w, h in ((392, 397), (392, 398), (393, 393), (393, 394))] == [155624, 156016, 155628, 156024]
    assert smc.SM_LDS_MAX == 155648


def test_names_and_counts():
    assert len(smc.BUILDERS) == len(set(smc.BUILDERS))
    groups = {n[0] for n in smc.BUILDERS}
    assert groups == set("abcdefgh")
    assert [n for n in smc.RAY_COUNTS] == [1, 63, 64, 65, 127, 128, 129, 4095, 4096]
    assert np.dtype(smc.get("a_d2").cells.dtype) == np.int8
