"""The chain's accumulator as the integer pair (key, M) (bl_serial_sum.h: ss_acc; bl_mcl_finish.h: mclf_chain) against the float
form it replaces, without a GPU.

Between list entries the chain keeps `key` (0x400 | sign << 9 | exponent field) and `M` (the 24-bit significand) and forms a float
only for the exact step, by integer operations on the bit pattern.  Held here, against bl_serial_sum.h's own ss_from (ldexpf) and
ss_rec_fits compiled for the host as tests/test_serial_sum_model.py compiles its model:
  * a numpy restatement of the bit-pattern form, and the header's ss_acc_float, give ss_from's bits for every key with exponent
    field 16..254, both signs, at M = 2^23, 2^23 + 1, 2^24 - 1, 2^24 (the carry into the exponent field) and 10 000 seeded M;
  * the gap application on the pair -- key compare, two adds and two compares on M, M += D -- accepts exactly what ss_rec_fits
    accepts and leaves ss_from(key, M + D): seeded records that fit, records that miss by one ulp at either end (and their
    neighbours that just fit), a wrong key, key 0 on either side, SS_ID."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MLO, MHI = 1 << 23, 1 << 24
SS_ID = 0x7FFFFFFF
KEYS = np.array([0x400 | (s << 9) | ex for s in (0, 1) for ex in range(16, 255)], np.int32)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("chain_state") / "chain_state_ref.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "cpp", "chain_state_ref.cpp")])
    return C.CDLL(so)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def bits_from_pair(key, M):
    """The float of (key, M), 2^23 <= M <= 2^24, from its bits: sign | (exponent field << 23) + (M - 2^23).  M = 2^24 carries into the
    exponent field: the next binade's first value, fraction zero."""
    key = key.astype(np.uint32)
    return ((key & np.uint32(0x200)) << np.uint32(22)) | (((key & np.uint32(0xFF)) << np.uint32(23)) + (M.astype(np.uint32) - np.uint32(MLO)))


def gap_on_pair(rec, key, M):
    """(fits, key, M) after the gap record rec = (key, D, lo, hi), on the pair alone."""
    rkey, D, lo, hi = (rec[:, k] for k in range(4))
    ident = rkey == SS_ID
    inside = (rkey == key) & (key != 0) & (M + lo > MLO) & (M + hi < MHI)
    return ident | inside, key, M + np.where(ident, 0, D)


def _grid(Ms):
    key = np.repeat(KEYS, len(Ms))
    M = np.tile(np.asarray(Ms, np.int32), len(KEYS))
    return key, M


def _from(ref, fn, key, M):
    out = np.zeros(len(key), np.uint32)
    getattr(ref, fn)(_p(np.ascontiguousarray(key, np.int32)), _p(np.ascontiguousarray(M, np.int32)), _p(out), len(key))
    return out


def test_bit_pattern_form_is_ss_from_at_the_binade_ends(ref):
    key, M = _grid([MLO, MLO + 1, MHI - 1, MHI])
    want = _from(ref, "csr_from", key, M)
    assert np.array_equal(bits_from_pair(key, M), want)
    assert np.array_equal(_from(ref, "csr_acc_float", key, M), want)
    # M = 2^24 is the next binade's first value (infinity from exponent field 254), never this binade with a zero fraction
    top = M == MHI
    ex = (key[top] & 0xFF).astype(np.uint32)
    assert np.array_equal((want[top] >> 23) & 0xFF, ex + 1) and np.all((want[top] & 0x7FFFFF) == 0)
    assert np.array_equal(want[top] >> 31, (key[top].astype(np.uint32) >> 9) & 1)


def test_bit_pattern_form_is_ss_from_on_seeded_magnitudes(ref):
    rng = np.random.default_rng(20)
    key, M = _grid(rng.integers(MLO, MHI + 1, 10_000))
    want = _from(ref, "csr_from", key, M)
    assert np.array_equal(bits_from_pair(key, M), want)
    assert np.array_equal(_from(ref, "csr_acc_float", key, M), want)


def test_pair_of_a_float_and_back(ref):
    """ss_acc_of then ss_acc_float is the identity on every float with a usable binade; key 0 for the others."""
    rng = np.random.default_rng(21)
    bits = np.concatenate([rng.integers(0, 1 << 32, 200_000, dtype=np.uint64).astype(np.uint32),
                           np.array([0, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 15 << 23, 16 << 23, (16 << 23) - 1, 0x7F7FFFFF], np.uint32)])
    key, M = np.zeros(len(bits), np.int32), np.zeros(len(bits), np.int32)
    ref.csr_acc_of(_p(bits), _p(key), _p(M), len(bits))
    ex = (bits >> 23) & 0xFF
    usable = (ex >= 16) & (ex != 255)
    assert np.array_equal(key != 0, usable)
    assert np.array_equal(_from(ref, "csr_acc_float", key[usable], M[usable]), bits[usable])
    assert np.array_equal(bits_from_pair(key[usable], M[usable]), bits[usable])


def _gap_cases():
    """(rec[n, 4], key[n], M[n], what[n])"""
    rng = np.random.default_rng(22)
    recs, keys, Ms, what = [], [], [], []

    def add(r, k, m, w):
        recs.append(r); keys.append(k); Ms.append(m); what.append(w)

    for key in KEYS:
        key = int(key)
        for _ in range(8):
            M = int(rng.integers(MLO + 2, MHI - 1))
            # a record that fits: lo <= D <= hi, M + lo > 2^23, M + hi < 2^24 (where the magnitude leaves room)
            lo = -int(rng.integers(0, max(M - MLO, 1)))
            hi = int(rng.integers(0, max(MHI - M, 1)))
            D = int(rng.integers(lo, hi + 1))
            add((key, D, lo, hi), key, M, "seeded")
            # the ends: lo / hi that reach the binade's end exactly (miss by one ulp) and stop one short of it (just fit)
            add((key, 0, MLO - M, 0), key, M, "lo_misses")
            add((key, 0, MLO + 1 - M, 0), key, M, "lo_fits")
            add((key, 0, 0, MHI - M), key, M, "hi_misses")
            add((key, 0, 0, MHI - 1 - M), key, M, "hi_fits")
            add((key, D, MLO + 1 - M, MHI - 1 - M), key, M, "both_ends_fit")
            add((key ^ 0x200, D, lo, hi), key, M, "wrong_sign")
            add((key + (1 if (key & 0xFF) < 254 else -1), D, lo, hi), key, M, "wrong_exponent")
            add((0, D, lo, hi), key, M, "record_key_0")
            add((SS_ID, 0, 0, 0), key, M, "identity")
    for _ in range(64):
        M = int(rng.integers(MLO, MHI))
        add((0, 0, 0, 0), 0, M, "both_keys_0")
        add((int(KEYS[3]), 0, 0, 0), 0, M, "acc_key_0")
    return np.array(recs, np.int64), np.array(keys, np.int64), np.array(Ms, np.int64), np.array(what)


def test_gap_on_the_pair_is_ss_rec_fits_then_ss_from(ref):
    rec, key, M, what = _gap_cases()
    n = len(key)
    fits = np.zeros(n, np.int32)
    out = np.zeros(n, np.uint32)
    ref.csr_gap(_p(np.ascontiguousarray(rec, np.int32)), _p(np.ascontiguousarray(key, np.int32)), _p(np.ascontiguousarray(M, np.int32)), _p(fits), _p(out), n)
    mfits, mkey, mM = gap_on_pair(rec, key, M)
    assert np.array_equal(mfits, fits != 0), what[mfits != (fits != 0)][:8]
    ok = fits != 0
    assert np.array_equal(bits_from_pair(mkey[ok], mM[ok]), out[ok])
    assert np.array_equal(_from(ref, "csr_acc_float", mkey[ok], mM[ok]), out[ok])
    # the cases are what they are called
    for name, want in (("seeded", True), ("lo_misses", False), ("lo_fits", True), ("hi_misses", False), ("hi_fits", True), ("both_ends_fit", True), ("wrong_sign", False),
                       ("wrong_exponent", False), ("record_key_0", False), ("identity", True), ("both_keys_0", False), ("acc_key_0", False)):
        sel = what == name
        assert sel.any() and np.all(ok[sel] == want), name
    # after a gap that fits the magnitude is strictly inside its binade: the pair needs no carry there
    assert np.all(mM[ok] > MLO) and np.all(mM[ok] < MHI)
