"""The conditions of tests/mapping_cases.py on the CPU: every hand-built input of tests/test_gpu_mapping_edges.py reaches the form of
k_map_update it is meant for, by the oracle's own arithmetic.  No GPU."""
import pytest

import mapping_cases as mc


@pytest.mark.parametrize("name", list(mc.BUILDERS))
def test_case_reaches_its_path(oracle, name):
    mc.evaluate(mc.get(name, oracle), oracle)


@pytest.mark.parametrize("form", ["pair", "one", "serial"])
def test_counter_cases_reach_their_path(oracle, form):
    for hit, miss in mc.SATURATION_ODDS:
        for shift in range(7):
            mc.evaluate(mc.counters(oracle, form, hit, miss, shift), oracle)
