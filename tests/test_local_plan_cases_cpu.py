"""tests/local_plan_cases.py on the CPU: every builder's own assertions hold (a case is what it is named for, by the model alone);
three mistaken selection rules -- ties to the highest c, the order (cost, i, j), the cost compared after truncation to int32 -- each
elect another winner than the definition on the cases of `ties` and `keys` that name them; and the emulation of how the kernels
spread a call over workgroups (local_plan_cases.emulate, the model's costs in place of the device's) equals the model, and stops
equalling it on a named case under each of four mistakes in that plumbing.

Wall time of this file on the CPU it was written on: 5 s, a third of it the two 64 x 9 x 255 rollouts of group `shapes`."""
import numpy as np
import pytest

import local_plan_cases as lc
import local_plan_model as lpm

RULES = ("ties_to_highest_c", "order_cost_i_j", "int32_cost")


@pytest.mark.parametrize("name", list(lc.BUILDERS))
def test_case_is_what_it_claims(name):
    factory, p, states = lc.get(name)
    assert len(states) == (66 if name.startswith("many") else 1)
    rec, cs, _ = lc.model((factory, p, states))
    assert len(cs) == p.n_v * p.n_w and int(rec["index"]) == lc.elect(cs) if int(rec["flags"]) == 0 else int(rec["index"]) == -1


def test_tables_of_the_groups():
    lc.check_shape_table()
    lc.check_theta_limit()
    assert sorted(n for g in lc.GROUPS.values() for n in g) == sorted(lc.BUILDERS)
    assert len(lc.SHAPE_RUNS) == 7 + 4 and all(k[2] >= 152 for k, v in lc.SHAPE_RUNS if v == 0.5)
    assert set(lc.DEFEATS) == set(lc.GROUPS["ties"] + lc.GROUPS["keys"])


@pytest.mark.parametrize("rule", RULES)
def test_a_mistaken_selection_rule_elects_another_winner(rule):
    named = [n for n, rules in lc.DEFEATS.items() if rule in rules]
    assert named, rule
    for name in lc.DEFEATS:
        case = lc.get(name)
        rec, cs, _ = lc.model(case)
        assert lc.elect(cs, "definition", case[1].n_v) == int(rec["index"]), name          # the rule spelled here is the model's
        differs = lc.elect(cs, rule, case[1].n_v) != int(rec["index"])
        assert differs == (rule in lc.DEFEATS[name]), (name, rule)


def test_where_the_tie_winners_sit():
    got = {n: lc.place(lc.get(n)[1], int(lc.model(lc.get(n))[0]["index"])) for n in lc.GROUPS["ties"]}
    print(got)
    assert [got[n][:2] for n in ("tie_wave1", "tie_wave2", "tie_wave3")] == [(0, 1), (0, 2), (0, 3)]
    assert [got[n][0] for n in ("tie_wg1", "tie_wg2", "tie_wg3", "tie_last_partial")] == [1, 2, 3, 3]
    assert got["tie_upper_half"][2] >= 32 and got["tie_baseline"][:2] == (0, 0)


# ---------------------------------------------------------------------------------------------------------------- the plumbing
def _two_calls(mistake):
    """many_first, then many_second on the same partials: the records of both calls"""
    partial = {}
    return [lc.emulate(lc.get(n), partial, mistake) for n in ("many_first", "many_second")]


def test_the_emulated_launch_equals_the_model():
    for got, name in zip(_two_calls(None), ("many_first", "many_second")):
        assert lc.same_records(got, lc.model_records(lc.get(name))), name
    for name in lc.SINGLE:
        case = lc.get(name)
        assert lc.same_records(lc.emulate(case, {}), lc.model_records(case)), name


# mistake -> the cases on which the emulated launch must stop equalling the model
CAUGHT_BY = {"ties_to_highest_c": ["tie_wave1", "tie_wg2", "tie_last_partial", "tie_baseline"], "narrow_products": ["keys"],
             "state_of_block": ["many_first"], "finish_reads_stale": ["many_second"]}


@pytest.mark.parametrize("mistake", list(CAUGHT_BY))
def test_a_mistake_in_the_plumbing_is_noticed(mistake):
    for name in CAUGHT_BY[mistake]:
        if name.startswith("many"):
            first, second = _two_calls(mistake)
            got = first if name == "many_first" else second
        else:
            got = lc.emulate(lc.get(name), {}, mistake)
        assert not lc.same_records(got, lc.model_records(lc.get(name))), (mistake, name)
