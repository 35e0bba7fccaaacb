"""The model of the loop-closure front end (bl_loopclose_find, include/botlab_hip.h, "loop closure").  TEST
INFRASTRUCTURE, no GPU.

The definition restated over the models that already exist: the pair rule in Python floats; the submaps through
map_rebuild_model.truth over the CPU oracle; the match through scan_match_prior_model.match; the gate; the edge in the header's
stated order, operation by operation in IEEE double (Python floats: no fused operation), with the pose graph's sincos32 and wrap.
The device must reproduce every field bit for bit.

edge_reference() is the formulation the Python path (botlab_amd.find_loop_closures) uses -- np.linalg.inv and atan2(sin, cos) -- for
the CPU test that measures how far the two formulations lie apart."""
import math

import numpy as np

import map_rebuild_model as mr
import pose_graph_model as pg
import scan_match_prior_model as smp

F32 = np.float32
NOT_ACCEPTED, TIED, ON_EDGE, TOO_MANY_RAYS = 1, 2, 4, 8
MAX_RAYS = 4096
MAX_CANDIDATES, MAX_W, MIN_SUBMAP, MAX_SUBMAP = 1024, 31, 16, 512

POSE_DTYPE = np.dtype([("utime", "<i8"), ("x", "<f4"), ("y", "<f4"), ("theta", "<f4"), ("pad", "<f4")])
RESULT_DTYPE = np.dtype([("pose", POSE_DTYPE), ("di", "<i4"), ("dj", "<i4"), ("dk", "<i4"), ("score", "<i4"), ("score_centre", "<i4"),
                         ("ties", "<i4"), ("rays_used", "<i4"), ("accepted", "<i4")])
MOMENTS_DTYPE = np.dtype([(n, "<i8") for n in smp.SUM_NAMES] + [("best_obj", "<i4"), ("pen_best", "<i4"), ("sub_num", "<i4", (3,)),
                                                                 ("sub_den", "<i4", (3,))])
EDGE_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("z", "<f8", (3,)), ("info", "<f8", (6,))])
CANDIDATE_DTYPE = np.dtype([("q", "<i4"), ("j", "<i4"), ("first", "<i4"), ("count", "<i4"), ("flags", "<u4"), ("pad", "<i4"),
                            ("result", RESULT_DTYPE), ("moments", MOMENTS_DTYPE), ("edge", EDGE_DTYPE)])
PARAMS_LAYOUT = (("stride", 0), ("min_gap", 4), ("radius", 8), ("w", 12), ("submap_cells", 16), ("max_laser", 20), ("hit", 24), ("miss", 28),
                 ("match", 32), ("prior", 60), (None, 84))
CANDIDATE_LAYOUT = (("q", 0), ("j", 4), ("first", 8), ("count", 12), ("flags", 16), ("pad", 20), ("result", 24), ("moments", 80), ("edge", 192),
                    (None, 272))

DEFAULTS = dict(stride=4, min_gap=40, radius=1.0, w=5, submap_cells=200, nx=8, ny=8, ntheta=12, dtheta=math.radians(0.5), max_range=8.0,
                half_life=64, min_score=0, maxLaserDistance=5.0, hitOdds=3, missOdds=1, prior=(0, 0, 0, 0))


def check_params(p):
    """True iff bl_loopclose_find accepts the parameters (a dict with DEFAULTS' keys)."""
    r = F32(p["radius"])
    if not (p["stride"] >= 1 and p["min_gap"] >= 0 and r > 0 and 0 <= p["w"] <= MAX_W and MIN_SUBMAP <= p["submap_cells"] <= MAX_SUBMAP):
        return False
    if not (0 <= p["hitOdds"] <= 127 and 0 <= p["missOdds"] <= 127):
        return False
    if not smp.sm.check_params(p["nx"], p["ny"], p["ntheta"], p["dtheta"]):
        return False
    return smp.check_prior(*p["prior"], half_life=p["half_life"], want_moments=True)


# ---------------------------------------------------------------- pairs
def d2_row(poses, q, last):
    """[d2(j) for j = 0 .. last]: the recorded float poses widened to double, every operation rounded by itself."""
    xq, yq = float(F32(poses[q][0])), float(F32(poses[q][1]))
    out = []
    for j in range(last + 1):
        dx, dy = float(F32(poses[j][0])) - xq, float(F32(poses[j][1])) - yq
        out.append(dx * dx + dy * dy)
    return out


def pairs(poses, stride, min_gap, radius):
    """[(q, j)] in ascending q: the lowest index of the minimum of d2 over j <= q - min_gap - 1, unless beyond the radius."""
    r = float(F32(radius))
    r2 = r * r
    out = []
    for q in range(0, len(poses), stride):
        last = q - min_gap - 1
        if last < 0:
            continue
        d2 = d2_row(poses, q, last)
        j = 0
        for k in range(1, last + 1):
            if d2[k] < d2[j]:
                j = k
        if d2[j] > r2:
            continue
        out.append((q, j))
    return out


# ---------------------------------------------------------------- submap, match, gate
def submap_origin(pose_j, S, mpc):
    half = F32(float(S) * float(F32(mpc)) / 2.0)
    return F32(F32(pose_j[0]) - half), F32(F32(pose_j[1]) - half)


def submap(orc, scans, poses, j, w, S, mpc, cpm, max_laser, hit, miss):
    """(cells int8 [S][S], origin, first, count) of the window around j."""
    n = len(poses)
    first, end = max(j - w, 0), min(j + w, n - 1)
    origin = submap_origin(poses[j], S, mpc)
    win = [(float(F32(p[0])), float(F32(p[1])), float(F32(p[2])), int(p[3])) for p in poses[first:end + 1]]
    cells = mr.truth(orc, scans[first:end + 1], win, None, np.zeros((S, S), np.int8), mpc, cpm, origin, max_laser, hit, miss)
    return cells, origin, first, end - first + 1


def gate(ref, nx, ny, ntheta):
    fl = 0
    if not ref["accepted"]:
        fl |= NOT_ACCEPTED
    if ref["ties"] != 1:
        fl |= TIED
    if not (abs(ref["di"]) < nx and abs(ref["dj"]) < ny and abs(ref["dk"]) < ntheta):
        fl |= ON_EDGE
    return fl


# ---------------------------------------------------------------- the edge
def _mul3(a, b):
    return [[(a[r][0] * b[0][c] + a[r][1] * b[1][c]) + a[r][2] * b[2][c] for c in range(3)] for r in range(3)]


def edge_parts(ref, centre, pose_j, mpc, dtheta):
    """(p, Sigma[6], s, c): the refined pose (float32 x, y, theta), the covariance, sine and cosine of theta_j as the pose graph forms them."""
    m, t = float(F32(mpc)), float(F32(dtheta))
    p = smp.refined_pose(ref, centre, m, t)
    _, cov = smp.covariance(ref["sums"], m, t)
    s, c = pg.sincos32(np.array([float(F32(pose_j[2]))]))
    return p, cov, float(s[0]), float(c[0])


def edge(ref, centre, pose_j, mpc, dtheta):
    """(z[3], info[6]) in the header's stated order of operations."""
    m, t = float(F32(mpc)), float(F32(dtheta))
    p, cov, s, c = edge_parts(ref, centre, pose_j, mpc, dtheta)
    xj, yj, tj = float(F32(pose_j[0])), float(F32(pose_j[1])), float(F32(pose_j[2]))
    dx, dy = float(p[0]) - xj, float(p[1]) - yj
    z = (c * dx + s * dy, c * dy - s * dx, float(pg.wrap(float(p[2]) - tj)))
    Sg = [[cov[0], cov[1], cov[3]], [cov[1], cov[2], cov[4]], [cov[3], cov[4], cov[5]]]
    Rt = [[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]]
    R = [[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]
    S = _mul3(_mul3(Rt, Sg), R)
    S[0][0] = S[0][0] + m * m / 12.0
    S[1][1] = S[1][1] + m * m / 12.0
    S[2][2] = S[2][2] + t * t / 12.0
    C = [[S[1][1] * S[2][2] - S[1][2] * S[2][1], S[1][2] * S[2][0] - S[1][0] * S[2][2], S[1][0] * S[2][1] - S[1][1] * S[2][0]],
         [S[0][2] * S[2][1] - S[0][1] * S[2][2], S[0][0] * S[2][2] - S[0][2] * S[2][0], S[0][1] * S[2][0] - S[0][0] * S[2][1]],
         [S[0][1] * S[1][2] - S[0][2] * S[1][1], S[0][2] * S[1][0] - S[0][0] * S[1][2], S[0][0] * S[1][1] - S[0][1] * S[1][0]]]
    det = (S[0][0] * C[0][0] + S[0][1] * C[0][1]) + S[0][2] * C[0][2]
    I = [[C[b][a] / det for b in range(3)] for a in range(3)]
    info = tuple(0.5 * (I[a][b] + I[b][a]) for a, b in ((0, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 2)))
    return z, info


def edge_reference(ref, centre, pose_j, mpc, dtheta):
    """(z[3], info[6]) as botlab_amd.find_loop_closures forms them: libm's cos / sin of the double heading, atan2(sin, cos), numpy's
    matrix products and np.linalg.inv."""
    m, t = float(F32(mpc)), float(F32(dtheta))
    p, cov, _, _ = edge_parts(ref, centre, pose_j, mpc, dtheta)
    tj = float(F32(pose_j[2]))
    c, sn = math.cos(tj), math.sin(tj)
    dx, dy = float(p[0]) - float(F32(pose_j[0])), float(p[1]) - float(F32(pose_j[1]))
    dth = float(p[2]) - tj
    z = (c * dx + sn * dy, -sn * dx + c * dy, math.atan2(math.sin(dth), math.cos(dth)))
    S = np.array([[cov[0], cov[1], cov[3]], [cov[1], cov[2], cov[4]], [cov[3], cov[4], cov[5]]])
    Rt = np.array([[c, sn, 0.0], [-sn, c, 0.0], [0.0, 0.0, 1.0]])
    S = Rt @ S @ Rt.T + np.diag([m * m / 12.0, m * m / 12.0, t ** 2 / 12.0])
    I = np.linalg.inv(S)
    I = 0.5 * (I + I.T)
    return z, (I[0, 0], I[0, 1], I[1, 1], I[0, 2], I[1, 2], I[2, 2])


# ---------------------------------------------------------------- the whole definition
def find(orc, scans, poses, mpc, cpm, **kw):
    """scans: the retained entries' LidarScans, oldest first; poses: their recorded (x, y, theta, utime).  Returns a list of
    candidates in ascending q, each a dict: q, j, first, count, flags, origin, cells, ref (scan_match_prior_model.match's dict, None
    with TOO_MANY_RAYS), z, info (None unless kept), d2 (the row of the pair search)."""
    p = dict(DEFAULTS, **kw)
    assert check_params(p)
    out = []
    for q, j in pairs(poses, p["stride"], p["min_gap"], p["radius"]):
        cells, origin, first, count = submap(orc, scans, poses, j, p["w"], p["submap_cells"], mpc, cpm, p["maxLaserDistance"], p["hitOdds"],
                                            p["missOdds"])
        c = dict(q=q, j=j, first=first, count=count, origin=origin, cells=cells, ref=None, z=None, info=None, flags=TOO_MANY_RAYS,
                 d2=d2_row(poses, q, q - p["min_gap"] - 1))
        centre = (F32(poses[q][0]), F32(poses[q][1]), F32(poses[q][2]))
        valid = len(smp.sm.valid_rays(scans[q].ranges, scans[q].thetas, p["max_range"])[0])
        c["valid"] = valid
        if valid <= MAX_RAYS:
            ref = smp.match(cells, origin, mpc, cpm, scans[q].ranges, scans[q].thetas, centre, p["nx"], p["ny"], p["ntheta"], p["dtheta"],
                            p["max_range"], prior=p["prior"], half_life=p["half_life"], min_score=p["min_score"], utime=int(poses[q][3]))
            c["ref"] = ref
            c["flags"] = gate(ref, p["nx"], p["ny"], p["ntheta"])
            if c["flags"] == 0:
                c["z"], c["info"] = edge(ref, centre, poses[j], mpc, p["dtheta"])
        out.append(c)
    return out


def records(cands):
    """CANDIDATE_DTYPE array of find()'s candidates: what bl_loopclose_candidates returns, byte for byte."""
    out = np.zeros(len(cands), CANDIDATE_DTYPE)
    for r, c in zip(out, cands):
        r["q"], r["j"], r["first"], r["count"], r["flags"] = c["q"], c["j"], c["first"], c["count"], c["flags"]
        ref = c["ref"]
        if ref is None:
            continue
        res, mom = r["result"], r["moments"]
        res["pose"]["utime"], res["pose"]["x"], res["pose"]["y"], res["pose"]["theta"] = ref["utime"], ref["x"], ref["y"], ref["theta"]
        for k in ("di", "dj", "dk", "score", "score_centre", "ties", "rays_used", "accepted"):
            res[k] = ref[k]
        for k, v in zip(smp.SUM_NAMES, ref["sums"]):
            mom[k] = v
        mom["best_obj"], mom["pen_best"] = ref["best_obj"], ref["pen_best"]
        mom["sub_num"] = [f[0] for f in ref["fractions"]]
        mom["sub_den"] = [f[1] for f in ref["fractions"]]
        if c["flags"] == 0:
            r["edge"]["i"], r["edge"]["j"], r["edge"]["z"], r["edge"]["info"] = c["j"], c["q"], c["z"], c["info"]
    return out


def edges(cands):
    rec = records(cands)
    return rec["edge"][rec["flags"] == 0].copy()
