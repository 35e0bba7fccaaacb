#!/usr/bin/env python3
"""Regenerates tests/golden/resample_parting_cases.npz: unequal-weight particle sets on which the kernels' default resampling rule
(the exact integer prefix, tests/resample_rule_model.py integer_rule) and the reference's rule (a sequentially rounded double
cumulative: the oracle's orc_resample_indices) choose different source particles -- and, per family of units, one rand() value at
which they do not.  Per case: N, the units, the rand() value, the oracle's indices, the model's indices.  The CPU test
tests/test_resample_rule_model_cpu.py regenerates both sides and holds them against the file; tests/test_gpu_uploaded_weights.py
holds the default mode against the model's side and strict mode against the oracle's."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import oracle_lib  # noqa: E402
import resample_rule_model as rrm  # noqa: E402


def generate(oracle):
    out = {"names": np.array([rrm.parting_name(*c) for c in rrm.PARTING_CASES]),
           "N": np.array([c[1] for c in rrm.PARTING_CASES], np.int32),
           "rand_value": np.array([c[2] for c in rrm.PARTING_CASES], np.int64)}
    for family, N, rv in rrm.PARTING_CASES:
        name = rrm.parting_name(family, N, rv)
        units = rrm.parting_units(family, N)
        out[name + "_units"] = units
        out[name + "_oracle"] = rrm.oracle_indices(oracle, units, rv)
        out[name + "_model"] = rrm.integer_rule(units, rv)
    return out


def main():
    np.savez_compressed(os.path.join(HERE, "resample_parting_cases.npz"), **generate(oracle_lib.load_oracle()))


if __name__ == "__main__":
    main()
