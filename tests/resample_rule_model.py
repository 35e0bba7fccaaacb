"""The default resampling rule of the kernels, stated once on the CPU (TEST INFRASTRUCTURE: nothing under botlab_amd/ imports this).

resamplePosteriorDistribution (particle_filter.cpp:84-103) compares U_m = r + m / M with a sequentially rounded double cumulative of
the normalised weights.  The kernels (k_mcl_main, k_pf_resample_only, k_pf_resample_next in bl_mcl.hip) compare U_m * S with the
EXACT integer prefix of the weight units instead:

    index(m) = first i with (r + m * (1 / M)) * S <= (double)prefix[i], clamped to N - 1

with M_inv = 1.0 / M, r = (rand_value / RAND_MAX) * M_inv, S = (double)sum(units), every operation a single IEEE double operation
(the library is built with -ffp-contract=off; numpy's ufuncs do not fuse either).  integer_rule() is that sentence and nothing else.
The reference's own rule is NOT restated here: it is the oracle's orc_resample_indices (oracle_indices() below only calls it).

PARTING_CASES / parting_units() name the unequal-weight sets on which the two rules provably part (by exactly one index, at some
rand() values and not at others); tests/golden/make_resample_parting_cases.py records both sides in
tests/golden/resample_parting_cases.npz."""
import numpy as np

from oracle_lib import PARTICLE_DTYPE

RAND_MAX = 2147483647
GLIBC = [1804289383, 846930886, 1681692777, 1714636915, 1957747793, 424238335, 719885386, 1649760492, 596516649, 1189641421,
         1025202362, 1350490027, 783368690, 1102520059, 2044897763, 1967513926]
EDGE = [0, 1, 1000, 1 << 30, RAND_MAX]



def integer_rule(units, rand_value, M=None):
    """Source index (int32) of each of the M output particles (M = N unless given: the adaptive count draws M from N records)."""
    u = [int(v) for v in np.asarray(units).ravel()]
    N = len(u)
    assert N >= 1 and min(u) >= 0
    M = N if M is None else int(M)
    prefix_int, run = [], 0
    for v in u:                                   # Python integers: no width, no rounding
        run += v
        prefix_int.append(run)
    assert 0 < run < (1 << 53), "the double conversion of the prefix is exact only below 2^53 (and a zero total has no weights)"
    prefix = np.array(prefix_int, dtype=np.uint64).astype(np.float64)
    assert all(int(p) == q for p, q in zip(prefix.tolist(), prefix_int))          # ... and it IS exact
    S = float(run)
    M_inv = 1.0 / M
    r = (float(rand_value) / float(RAND_MAX)) * M_inv
    T = (r + np.arange(M, dtype=np.float64) * M_inv) * S                          # one rounding per operation, as in the kernels
    return np.minimum(np.searchsorted(prefix, T, side="left"), N - 1).astype(np.int32)


def weights_of(units):
    """The weights the library hands out for these units (k_pf_export): (double)units / (double)S."""
    u = np.asarray(units, dtype=np.uint64)
    total = sum(int(v) for v in u.tolist())
    assert 0 < total < (1 << 53)
    return u.astype(np.float64) / float(total)


def oracle_indices(oracle, units=None, rand_value=0, particles=None):
    """orc_resample_indices on `particles` (a PARTICLE_DTYPE array), or on particles that carry weights_of(units)."""
    if particles is None:
        particles = np.zeros(len(units), PARTICLE_DTYPE)
        particles["weight"] = weights_of(units)
    p = np.ascontiguousarray(particles)
    assert p.dtype.itemsize == 56
    out = np.empty(p.size, np.int32)
    oracle.lib.orc_resample_indices(p.ctypes.data, int(p.size), int(rand_value), out.ctypes.data)
    return out


# ---- the committed parting cases: (family, N, rand() value).  A family is a tile of unequal units; every family has rand() values
# at which the rules part and one at which nothing parts.
PARTING_FAMILIES = {"alt2": [1000, 3000], "alt3": [1000, 3000, 5000]}
PARTING_CASES = ([("alt2", N, rv) for N in (200, 1000) for rv in (0, RAND_MAX, 1000)] +
                 [("alt3", 12345, rv) for rv in (0, 1, RAND_MAX, 1804289383)])


def parting_units(family, N):
    tile = PARTING_FAMILIES[family]
    assert N % len(tile) == 0
    return np.tile(np.array(tile, np.uint32), N // len(tile))


def parting_name(family, N, rv):
    return f"{family}_{N}_{rv}"
