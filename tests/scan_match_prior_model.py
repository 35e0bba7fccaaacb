"""The model of the scan match with a prior: a numpy / Python-integer restatement of "correlative scan matching with a prior" in
include/botlab_hip.h over tests/scan_match_model.py, which bl_scanmatch_match_prior (botlab_amd/csrc/bl_scanmatch.hip) must
reproduce byte for byte: the result struct, the ten sums, best_obj, pen_best, the sub-cell fractions and the objective volume.

Everything compared or summed is an integer; the two helpers in double (covariance, refined_pose) restate the header's
static inline functions operation by operation in Python floats (IEEE double, no fused operations)."""
import math
import os
import re
from fractions import Fraction

import numpy as np

import scan_match_model as sm

F32 = np.float32
MAX_COEFF = 32767
MAX_HALF_LIFE = 1 << 20
OBJ_BIAS = 1 << 23
SUM_NAMES = ("s0", "sx", "sy", "st", "sxx", "sxy", "syy", "sxt", "syt", "stt")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def exp2_entry(i):
    """floor(2^20 2^(-i/64)) in integers: the n with n^64 2^i <= 2^1280 < (n + 1)^64 2^i."""
    lo, hi = 0, 1 << 21
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if mid ** 64 * 2 ** i <= 2 ** 1280:
            lo = mid
        else:
            hi = mid
    return lo


EXP2 = [exp2_entry(i) for i in range(64)]


def header_table():
    """The 64 literals of BL_SM_EXP2_VALUES as include/botlab_hip.h writes them."""
    text = open(os.path.join(ROOT, "include", "botlab_hip.h")).read()
    body = re.search(r"#define BL_SM_EXP2_VALUES((?:.*\\\n)*.*)\n", text).group(1)
    return [int(v) for v in re.findall(r"\d+", body)]


def check_prior(a_xx, a_xy, a_yy, a_tt, half_life=None, want_moments=False, moments_given=True):
    """True iff bl_scanmatch_match_prior accepts the prior (the window's limits are sm.check_params')."""
    if not (0 <= a_xx <= MAX_COEFF and 0 <= a_yy <= MAX_COEFF and 0 <= a_tt <= MAX_COEFF and -MAX_COEFF <= a_xy <= MAX_COEFF):
        return False
    if a_xy * a_xy > a_xx * a_yy:
        return False
    if want_moments and not (half_life is not None and 1 <= half_life <= MAX_HALF_LIFE and moments_given):
        return False
    return True


def pen_volume(prior, nx, ny, ntheta):
    """int64 [2 ntheta + 1][2 ny + 1][2 nx + 1] of pen(di, dj, dk)."""
    a_xx, a_xy, a_yy, a_tt = (int(v) for v in prior)
    di = np.arange(-nx, nx + 1, dtype=np.int64)[None, None, :]
    dj = np.arange(-ny, ny + 1, dtype=np.int64)[None, :, None]
    dk = np.arange(-ntheta, ntheta + 1, dtype=np.int64)[:, None, None]
    q = a_xx * di * di + 2 * a_xy * di * dj + a_yy * dj * dj + a_tt * dk * dk
    assert q.min() >= 0 and q.max() < 2 ** 31
    return q >> 8


def pen(prior, di, dj, dk):
    a_xx, a_xy, a_yy, a_tt = (int(v) for v in prior)
    return (a_xx * di * di + 2 * a_xy * di * dj + a_yy * dj * dj + a_tt * dk * dk) >> 8


def best_candidate(obj, nx, ny, ntheta):
    """Highest objective, then sm.best_candidate's order.  Returns (di, dj, dk, best_obj, ties)."""
    return sm.best_candidate(obj, nx, ny, ntheta)


def weight(d, half_life):
    e = d // half_life
    f = d - e * half_life
    i = (64 * f) // half_life
    return 0 if e >= 21 else EXP2[i] >> e


def weights(obj, best_obj, half_life):
    """int64 array of w, the definition's integer divisions on numpy int64."""
    d = np.int64(best_obj) - obj.astype(np.int64)
    assert d.min() >= 0 and d.max() < 2 ** 24
    e = d // half_life
    f = d - e * half_life
    i = (64 * f) // half_life
    tab = np.array(EXP2, dtype=np.int64)
    return np.where(e >= 21, 0, tab[i] >> np.minimum(e, 63))


def moment_sums(obj, best_obj, half_life, nx, ny, ntheta):
    """The ten sums as Python integers, in SUM_NAMES' order."""
    w = weights(obj, best_obj, half_life)
    di = np.arange(-nx, nx + 1, dtype=np.int64)[None, None, :]
    dj = np.arange(-ny, ny + 1, dtype=np.int64)[None, :, None]
    dk = np.arange(-ntheta, ntheta + 1, dtype=np.int64)[:, None, None]
    terms = (w, w * di, w * dj, w * dk, w * di * di, w * di * dj, w * dj * dj, w * di * dk, w * dj * dk, w * dk * dk)
    out = tuple(int(t.sum(dtype=np.int64)) for t in terms)             # below 2^58: int64 is exact
    assert out[0] >= 1 << 20
    return out


def sub_cell(obj, di, dj, dk, nx, ny, ntheta):
    """((num, den) for x, y, t)."""
    at = (dk + ntheta, dj + ny, di + nx)
    o0 = int(obj[at])
    out = []
    for axis, pos, half in ((2, di, nx), (1, dj, ny), (0, dk, ntheta)):
        num, den = 0, 1
        if half >= 1 and -half < pos < half:
            lo, hi = list(at), list(at)
            lo[axis] -= 1
            hi[axis] += 1
            om, op = int(obj[tuple(lo)]), int(obj[tuple(hi)])
            den, num = 2 * (2 * o0 - om - op), op - om
            if den == 0:
                num, den = 0, 1
        out.append((num, den))
    return tuple(out)


def match(cells, origin, mpc, cpm, scan_ranges, scan_thetas, centre, nx, ny, ntheta, dtheta, max_range, prior=(0, 0, 0, 0),
          half_life=None, min_score=0, utime=0):
    """The whole definition.  Returns sm.match's dict -- "score" the raw score of the winner, "ties" on the objective, "volume"
    the OBJECTIVE volume (int32) -- and, with half_life, "sums" (SUM_NAMES' order), "best_obj", "pen_best", "fractions"."""
    assert check_prior(*prior, half_life=half_life, want_moments=half_life is not None)
    ref = sm.match(cells, origin, mpc, cpm, scan_ranges, scan_thetas, centre, nx, ny, ntheta, dtheta, max_range, min_score=min_score,
                   utime=utime)
    score = ref["volume"].astype(np.int64)
    obj = score - pen_volume(prior, nx, ny, ntheta)
    assert -OBJ_BIAS < obj.min() and obj.max() < 2 ** 19
    di, dj, dk, best_obj, ties = best_candidate(obj, nx, ny, ntheta)
    raw = int(score[dk + ntheta, dj + ny, di + nx])
    assert raw == best_obj + pen(prior, di, dj, dk)
    accepted = int(raw >= min_score)
    c = (F32(centre[0]), F32(centre[1]), F32(centre[2]))
    if accepted:
        x = F32(float(c[0]) + di * float(F32(mpc)))
        y = F32(float(c[1]) + dj * float(F32(mpc)))
        theta = sm.wrap_to_pi(F32(c[2] + F32(F32(dk) * F32(dtheta))))
    else:
        x, y, theta = c
    out = dict(ref, x=F32(x), y=F32(y), theta=F32(theta), di=di, dj=dj, dk=dk, score=raw, ties=ties, accepted=accepted,
               volume=obj.astype(np.int32), score_volume=ref["volume"], raw_best=sm.best_candidate(ref["volume"], nx, ny, ntheta))
    if half_life is not None:
        out.update(sums=moment_sums(obj, best_obj, half_life, nx, ny, ntheta), best_obj=int(best_obj), pen_best=pen(prior, di, dj, dk),
                   fractions=sub_cell(obj, di, dj, dk, nx, ny, ntheta))
    return out


# ---------------------------------------------------------------------------------------------------------------- helpers
def covariance_exact(sums, meters_per_cell, dtheta):
    """(mean[3], cov[6]) as Fractions; the scales are the doubles given, taken exactly."""
    s0, sx, sy, st, sxx, sxy, syy, sxt, syt, stt = (Fraction(v) for v in sums)
    m, t = Fraction(float(meters_per_cell)), Fraction(float(dtheta))
    mx, my, mt = sx / s0, sy / s0, st / s0
    cov = ((sxx / s0 - mx * mx) * m * m, (sxy / s0 - mx * my) * m * m, (syy / s0 - my * my) * m * m, (sxt / s0 - mx * mt) * m * t,
           (syt / s0 - my * mt) * m * t, (stt / s0 - mt * mt) * t * t)
    return (mx * m, my * m, mt * t), cov


def covariance_terms(sums, meters_per_cell, dtheta):
    """For each cov entry (|E[ab]|, |E[a] E[b]|, scale) as floats: what the tolerance of the double helper is built from."""
    s0, sx, sy, st, sxx, sxy, syy, sxt, syt, stt = (Fraction(v) for v in sums)
    m, t = float(meters_per_cell), float(dtheta)
    mx, my, mt = sx / s0, sy / s0, st / s0
    rows = ((sxx, mx, mx, m * m), (sxy, mx, my, m * m), (syy, my, my, m * m), (sxt, mx, mt, m * t), (syt, my, mt, m * t), (stt, mt, mt, t * t))
    return [(abs(float(sab / s0)), abs(float(a * b)), abs(s)) for sab, a, b, s in rows]


def covariance(sums, meters_per_cell, dtheta):
    """bl_scanmatch_covariance in Python floats, operation by operation."""
    s0, sx, sy, st, sxx, sxy, syy, sxt, syt, stt = (float(v) for v in sums)
    m, t = float(meters_per_cell), float(dtheta)
    mx, my, mt = sx / s0, sy / s0, st / s0
    return ((mx * m, my * m, mt * t),
            ((sxx / s0 - mx * mx) * (m * m), (sxy / s0 - mx * my) * (m * m), (syy / s0 - my * my) * (m * m),
             (sxt / s0 - mx * mt) * (m * t), (syt / s0 - my * mt) * (m * t), (stt / s0 - mt * mt) * (t * t)))


def refined_pose(ref, centre, meters_per_cell, dtheta):
    """bl_scanmatch_refined_pose in Python floats: (x, y, theta) as float32."""
    if not ref["accepted"]:
        return F32(ref["x"]), F32(ref["y"]), F32(ref["theta"])
    (nx_, dx_), (ny_, dy_), (nt_, dt_) = ref["fractions"]
    m, t = float(meters_per_cell), float(dtheta)
    x = F32(float(F32(centre[0])) + (float(ref["di"]) + float(nx_) / float(dx_)) * m)
    y = F32(float(F32(centre[1])) + (float(ref["dj"]) + float(ny_) / float(dy_)) * m)
    th = F32(float(F32(centre[2])) + (float(ref["dk"]) + float(nt_) / float(dt_)) * t)
    return x, y, sm.wrap_to_pi(th)


def prior_from_sigmas(sigma_x, sigma_y, rho, sigma_theta, score_per_nat, meters_per_cell, dtheta):
    """botlab_amd.prior_from_sigmas' rule restated with exact rationals where the double result is not in doubt: used by the CPU
    test on inputs whose products are exact in double (powers of two and small integers)."""
    k = Fraction(128) * Fraction(score_per_nat)
    sx, sy, st = Fraction(sigma_x) / Fraction(meters_per_cell), Fraction(sigma_y) / Fraction(meters_per_cell), Fraction(sigma_theta) / Fraction(dtheta)
    q = 1 - Fraction(rho) ** 2

    def coeff(v, lo):
        return int(math.floor(min(max(v, lo), Fraction(MAX_COEFF)) + Fraction(1, 2)))
    a_xx, a_yy, a_tt = coeff(k / (q * sx * sx), 0), coeff(k / (q * sy * sy), 0), coeff(k / (st * st), 0)
    a_xy = coeff(-k * Fraction(rho) / (q * sx * sy), -MAX_COEFF)
    if a_xy * a_xy > a_xx * a_yy:
        a_xy = int(math.copysign(math.isqrt(a_xx * a_yy), a_xy))
    return a_xx, a_xy, a_yy, a_tt
