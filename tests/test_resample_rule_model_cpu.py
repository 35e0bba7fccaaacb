"""tests/resample_rule_model.py integer_rule (the kernels' default resampling rule, restated) against the oracle's
orc_resample_indices (the reference's rule):
  * on weights as an update leaves them the two rules choose the same source for every rand() value of the GPU sweep
    (tests/test_gpu_resample_sweep.py asserts the same of the kernels): the model is the oracle there, index for index;
  * on the committed unequal-weight sets (tests/golden/resample_parting_cases.npz) they part, always by exactly one index, at the
    rand() values recorded there and nowhere else.  The file is regenerated here, both sides, and must come out the same.
No GPU."""
import importlib.util
import os

import numpy as np
import pytest

import resample_rule_model as rrm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_resample_parting_cases", os.path.join(GOLDEN, "make_resample_parting_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("N", [200, 4096])
def test_model_equals_the_oracle_on_update_like_weights(oracle, N):
    rng = np.random.default_rng(7 * N)                        # the weights of test_resample_index_disagreements_are_counted_and_bounded
    units = (1000 * rng.integers(40, 36000, N)).astype(np.uint32)
    units[rng.random(N) < 0.02] = 2
    converged = (1000 * rng.integers(30000, 30400, N)).astype(np.uint32)
    for kind, u in (("after_update", units), ("converged", converged)):
        for rv in rrm.EDGE + rrm.GLIBC:
            assert np.array_equal(rrm.integer_rule(u, rv), rrm.oracle_indices(oracle, u, rv)), (kind, N, rv)


def test_model_takes_integers_of_any_size_and_refuses_what_a_double_cannot_hold():
    # Python integers, numpy integers of any width; a total of 2^53 or more would round in the kernels' conversion
    assert np.array_equal(rrm.integer_rule([0xFFFFFFFF] * 5 + [1], 1 << 30), rrm.integer_rule(np.array([0xFFFFFFFF] * 5 + [1], np.uint64), 1 << 30))
    assert np.array_equal(rrm.integer_rule([0, 0, 7], 0), [0, 2, 2])                  # T_0 = 0 is reached by a zero prefix (the reference: U > c fails at 0 > 0)
    assert np.array_equal(rrm.integer_rule([0, 0, 7], 1), [2, 2, 2])
    assert np.array_equal(rrm.integer_rule([7, 0, 0], 1 << 30), [0, 0, 0])
    assert np.array_equal(rrm.integer_rule([1, 1, 1, 1], 1 << 30, M=2), [1, 3])       # two drawn from four: U just above 1/4, 3/4
    with pytest.raises(AssertionError):
        rrm.integer_rule([1 << 52, 1 << 52], 0)
    with pytest.raises(AssertionError):
        rrm.integer_rule([0, 0, 0], 0)


def test_committed_parting_cases_regenerate_and_part_by_one_index(oracle):
    fresh = _generator().generate(oracle)
    with np.load(os.path.join(GOLDEN, "resample_parting_cases.npz")) as z:
        held = {k: z[k] for k in z.files}
    assert sorted(fresh) == sorted(held)
    for k in fresh:
        assert fresh[k].dtype == held[k].dtype and np.array_equal(fresh[k], held[k]), k
    assert [str(n) for n in held["names"]] == [rrm.parting_name(*c) for c in rrm.PARTING_CASES]
    parted, quiet = {}, set()
    for (family, N, rv), name in zip(rrm.PARTING_CASES, held["names"]):
        o, m = held[f"{name}_oracle"].astype(np.int64), held[f"{name}_model"].astype(np.int64)
        assert o.size == N and m.size == N and held[f"{name}_units"].size == N
        d = np.nonzero(o != m)[0]
        assert np.all(np.abs(o[d] - m[d]) == 1), name                     # every difference is exactly one index
        if d.size:
            parted[str(name)] = int(d.size)
        else:
            quiet.add(family)
    assert len(parted) >= 3, parted                                       # the fixture has not degenerated into "nothing parts"
    assert quiet == set(rrm.PARTING_FAMILIES), quiet                      # ... and every family has a rand() value at which nothing does
    assert any(N >= 4096 and (N & (N - 1)) for _, N, _ in rrm.PARTING_CASES)
