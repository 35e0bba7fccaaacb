"""The model of the local planner's moving rule and of the static composition (include/botlab_hip.h, "local planner, moving
obstacles" and bl_obstracks_compose_static), restated in Python over tests/local_plan_model.py and tests/obstacle_tracks_model.py:
what bl_localplan_commands_moving, bl_localplan_debug_costs_moving and bl_obstracks_compose_static are checked against, byte for
byte.  Written from the definition: every used slot is tested at every step -- no reach cull, no table of boxes.
"""
import math

import numpy as np

import local_plan_model as lpm
import obstacle_tracks_model as tm
from obstacle_layer_model import StateError

F32 = np.float32
MOVING_BYTES = 10 * 1024                                     # BL_LOCALPLAN_MOVING_BYTES
MAX_MARGIN = 64
POS_MAX = 1 << 30
PATH_TABLE, PATH_PER_STEP, PATH_NONE = 0, 1, 2


class Moving:
    """bl_localplan_moving_t"""

    def __init__(self, steps_per_update, margin_cells=0, lead_steps=0, reserved=0):
        self.q, self.margin, self.lead, self.reserved = int(steps_per_update), int(margin_cells), int(lead_steps), int(reserved)

    def ok(self):
        return 1 <= self.q <= 255 and 0 <= self.margin <= MAX_MARGIN and 0 <= self.lead <= 255 and self.reserved == 0


def used(slot):
    """The used-slot predicate, on the flags as they stand in the slot."""
    f = int(slot["flags"])
    want = tm.CONFIRMED | tm.MOVING
    return int(slot["id"]) != 0 and (f & want) == want and (f & (tm.MATCHED | tm.BORN)) != 0


def used_slots(slots):
    return [s for s in slots if used(s)]


def offset(t, v, q):
    """floor((t v + 128 q) / (256 q)) -- Python's // rounds towards minus infinity"""
    return (t * v + 128 * q) // (256 * q)


def box_at(slot, k, m):
    """(x0, y0, x1, y1), inclusive, of a used slot at rollout step k (1 .. n_steps)."""
    c = [tm.clamp(int(slot[n]), -POS_MAX, POS_MAX) for n in ("x0", "y0", "x1", "y1")]
    t = k + m.lead
    ox, oy = offset(t, int(slot["vx"]), m.q), offset(t, int(slot["vy"]), m.q)
    return c[0] + ox - m.margin, c[1] + oy - m.margin, c[2] + ox + m.margin, c[3] + oy + m.margin


def in_box(box, cell):
    return box[0] <= cell[0] <= box[2] and box[1] <= cell[1] <= box[3]


def cells_of(world, p, pose, v, w):
    """Per candidate c = j * n_v + i the visited cells [cell_1 .. cell_n], None where the pose has none.  The arithmetic of
    lpm.costs, the n_v speeds of a heading taken together as a float32 array (one rounding per operation either way)."""
    vt, wt = lpm.tables(p, v, w)
    out = [None] * (p.n_w * p.n_v)
    s = (vt * p.dt_sim).astype(np.float32)
    for j in range(p.n_w):
        cs_sn = lpm.trig(lpm.headings(pose[2], wt[j], p.dt_sim, p.n_steps)[:-1])
        x, y = np.full(p.n_v, F32(pose[0]), np.float32), np.full(p.n_v, F32(pose[1]), np.float32)
        rows = [[] for _ in range(p.n_v)]
        for k in range(p.n_steps):
            x = x + s * cs_sn[k][0]
            y = y + s * cs_sn[k][1]
            assert x.dtype == np.float32 and y.dtype == np.float32
            for i in range(p.n_v):
                rows[i].append(world.cell(x[i], y[i]))
        for i in range(p.n_v):
            out[j * p.n_v + i] = rows[i]
    return out


def first_hit(world, p, slots, m, pose, v, w, cells=None):
    """int32 [n_w * n_v]: the least k whose visited cell lies in a used slot's box at step k, 0 when there is none; every k whose
    pose has a cell is looked at."""
    us = used_slots(slots)
    out = np.zeros(p.n_w * p.n_v, np.int32)
    if not us:
        return out
    boxes = [[box_at(s, k, m) for s in us] for k in range(1, p.n_steps + 1)]
    cells = cells if cells is not None else cells_of(world, p, pose, v, w)
    for c, row in enumerate(cells):
        for k, cell in enumerate(row):
            if cell is not None and any(in_box(b, cell) for b in boxes[k]):
                out[c] = k + 1
                break
    return out


def costs_moving(world, p, slots, m, pose, v, w, stats=None):
    """(costs, first_hit): lpm.costs with the candidates that meet a moving box made inadmissible."""
    assert m.ok()
    fh = first_hit(world, p, slots, m, pose, v, w)
    cs = lpm.costs(world, p, pose, v, w)
    if stats is not None:
        stats["hit"] = stats.get("hit", 0) + int(np.count_nonzero(fh))
        stats["hit_only"] = stats.get("hit_only", 0) + int(np.count_nonzero((fh > 0) & (cs != lpm.COST_NONE)))
    return np.where(fh > 0, lpm.COST_NONE, cs).astype(np.int64), fh


def command_moving(world, p, slots, m, pose, v, w, stats=None):
    """The RESULT record of one state under the moving rule, the costs and first_hit (None, None when nothing was rolled out)."""
    assert lpm.state_ok(pose, v, w) and m.ok()
    r = np.zeros((), lpm.RESULT)
    r["index"], r["cost"] = -1, lpm.COST_NONE
    flags = world.start_flags(pose[0], pose[1])              # on the pose's own cell alone, before anything is rolled out
    if flags:
        r["flags"] = flags
        if flags == lpm.REACHED:
            r["cost"] = 0
        return r, None, None
    cs, fh = costs_moving(world, p, slots, m, pose, v, w, stats)
    adm = cs != lpm.COST_NONE
    r["n_admissible"] = int(adm.sum())
    if not adm.any():
        r["flags"] = lpm.BLOCKED
        return r, cs, fh
    c = int(np.argmin(cs))
    vt, wt = lpm.tables(p, v, w)
    r["index"], r["cost"] = c, int(cs[c])
    r["trans_v"], r["angular_v"] = vt[c % p.n_v], wt[c // p.n_v]
    return r, cs, fh


def refusal(world, p, m, tracker_shape, states):
    """What bl_localplan_commands_moving answers before it launches anything: None, or the reason it is BL_ERR_ARG."""
    if not 1 <= m.q <= 255:
        return "steps_per_update"
    if not 0 <= m.margin <= MAX_MARGIN:
        return "margin_cells"
    if not 0 <= m.lead <= 255:
        return "lead_steps"
    if m.reserved != 0:
        return "reserved"
    if p.can_skip_a_cell(world.mpc):
        return "step skips a cell"
    if not all(lpm.state_ok(*s) for s in states):
        return "state"
    if tuple(tracker_shape) != (world.w, world.h):
        return "tracker shape"
    return None


# ---------------------------------------------------------------------------------------------------------------- what the device does
def reach(p, cpm):
    """R of the window rule."""
    return int(math.ceil(p.v_abs() * float(p.dt_sim) * p.n_steps * float(F32(cpm)))) + 2


def kept_slots(world, p, slots, m, pose):
    """The used slots whose box swept over k = 1 .. n_steps meets the reach square around the window's centre: the device's cull,
    restated so that the tests can tell which path a call must take.  It decides speed only -- the model above does not cull."""
    R = reach(p, world.cpm)
    vx = (float(F32(pose[0])) - float(F32(world.origin[0]))) * float(world.cpm)
    vy = (float(F32(pose[1])) - float(F32(world.origin[1]))) * float(world.cpm)
    ccx, ccy = int(min(max(vx, 0.0), world.w - 1.0)), int(min(max(vy, 0.0), world.h - 1.0))
    out = []
    for s in used_slots(slots):
        a, b = box_at(s, 1, m), box_at(s, p.n_steps, m)
        lx, hx, ly, hy = min(a[0], b[0]), max(a[2], b[2]), min(a[1], b[1]), max(a[3], b[3])
        if hx >= ccx - R and lx <= ccx + R and hy >= ccy - R and ly <= ccy + R:
            out.append(s)
    return out


def moving_path(world, p, slots, m, pose):
    kept = len(kept_slots(world, p, slots, m, pose))
    return PATH_NONE if kept == 0 else PATH_TABLE if kept * p.n_steps * 8 <= MOVING_BYTES else PATH_PER_STEP


# ---------------------------------------------------------------------------------------------------------------- the composition
def compose_static(tracker, layer_live, layer_n, cells):
    """bl_obstracks_compose_static over a tm.Tracker: 127 where the layer is live, except the cells of the last update's blobs that
    were matched to or born as a CONFIRMED and MOVING track, which keep the map's value."""
    if not tracker.fresh and layer_n != tracker.n:
        raise StateError("order")
    cells = np.asarray(cells, np.int8)
    out = cells.copy()
    out[np.asarray(layer_live, bool)] = 127
    want = tm.CONFIRMED | tm.MOVING
    for (x, y), lab in zip(tracker.live_xy.tolist(), tracker.labels.tolist()):
        if lab < 0 or tracker.blobs["track"][lab] < 0:
            continue
        if (int(tracker.slots[tracker.blobs["track"][lab]]["flags"]) & want) == want:
            out[y, x] = cells[y, x]
    return out


def make_slot(id, x0, y0, x1, y1, vx=0, vy=0, flags=tm.CONFIRMED | tm.MOVING | tm.MATCHED, hits=5):
    """A slot record as bl_obstracks_upload takes it: the position is the box's centre."""
    s = np.zeros((), tm.TRACK_DTYPE)
    px, py = 128 * (int(x0) + int(x1) + 1), 128 * (int(y0) + int(y1) + 1)
    s["id"], s["px"], s["py"] = id, tm.clamp(px, -POS_MAX, POS_MAX), tm.clamp(py, -POS_MAX, POS_MAX)
    s["vx"], s["vy"], s["hits"], s["flags"] = vx, vy, hits, flags
    s["x0"], s["y0"], s["x1"], s["y1"] = x0, y0, x1, y1
    s["area"] = 1
    return s


def slot_table(records):
    """All 256 slots with `records` (slot index -> record, or a list from slot 0 on) placed."""
    out = np.zeros(tm.MAX_TRACKS, tm.TRACK_DTYPE)
    out["slot"] = np.arange(tm.MAX_TRACKS)
    items = records.items() if isinstance(records, dict) else enumerate(records)
    for i, r in items:
        out[i] = r
        out["slot"][i] = i
    return out
