"""The model of the likelihood field (include/botlab_hip.h, "likelihood field"), restated in Python: the definition the kernels of
botlab_amd/csrc/bl_lfield.hip are checked against, cell for cell.

  codes        the capped squared distance to the nearest source (log-odds >= occ_min): tests/edt_model.py applied to
               np.where(cells >= occ_min, 0, -1), with FAR = R^2 + 1 everywhere when the map has no source
  table_exact  the unrounded table values peak * exp(-(k m^2) / (2 s^2)) in double, with math.exp -- the C library's exp, which is
               what the library calls, not numpy's vectorised one
  table        T[k] = (int8) floor(that + 0.5), k = 0 .. R^2;  T[R^2 + 1] = 0
  near_half    does any unrounded value lie within 1e-6 of a half-integer?  (There a last-bit difference between two exp
               implementations could change an entry; the tests assert that the parameters they use stay clear of it.)
  field        THE MODEL: T[codes]
  brute_force  a second, independent form: every cell against every source
"""
import math

import numpy as np

import edt_model as em

MAX_CELLS = 64


def far(R):
    return R * R + 1


def codes(cells, R, occ_min):
    """int64 (h, w): d2 when d2 <= R^2, else FAR; FAR everywhere without a source."""
    cells = np.asarray(cells)
    c = em.codes(np.where(cells >= occ_min, 0, -1).astype(np.int8), R).astype(np.int64)
    return np.where(c == em.NONE16, far(R), c)


def table_exact(sigma, R, mpc, peak):
    m, s = float(np.float32(mpc)), float(np.float32(sigma))
    return [float(peak) * math.exp(-(float(k) * (m * m)) / (2.0 * (s * s))) for k in range(R * R + 1)]


def table(sigma, R, mpc, peak):
    """int8 [R^2 + 2]."""
    assert 1 <= R <= MAX_CELLS and 1 <= peak <= 127
    t = [math.floor(v + 0.5) for v in table_exact(sigma, R, mpc, peak)] + [0]
    return np.array(t, dtype=np.int8)


def near_half(sigma, R, mpc, peak, eps=1e-6):
    return any(abs((v - math.floor(v)) - 0.5) <= eps for v in table_exact(sigma, R, mpc, peak))


def field(cells, sigma, R, mpc, occ_min=1, peak=127):
    """THE MODEL.  int8 (h, w)."""
    assert 1 <= occ_min <= 127
    return table(sigma, R, mpc, peak)[codes(cells, R, occ_min)]


def brute_force(cells, sigma, R, mpc, occ_min=1, peak=127):
    """The same field from the definition: the minimum over all sources, cell by cell, and the formula of an entry."""
    cells = np.asarray(cells)
    h, w = cells.shape
    ys, xs = np.nonzero(cells >= occ_min)
    out = np.zeros((h, w), np.int8)
    if len(xs) == 0:
        return out
    xs, ys = xs.astype(np.int64), ys.astype(np.int64)
    m, s = float(np.float32(mpc)), float(np.float32(sigma))
    for y in range(h):
        for x in range(w):
            d2 = int(((xs - x) ** 2 + (ys - y) ** 2).min())
            if d2 <= R * R:
                out[y, x] = math.floor(float(peak) * math.exp(-(float(d2) * (m * m)) / (2.0 * (s * s))) + 0.5)
    return out
