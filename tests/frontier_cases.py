"""Hand-built maps for find_map_frontiers (bl_frontiers.hip) and a small numpy model of the search that serves ONLY the conditions:
which level path, which growth path, which table a map reaches.  The expected frontier lists come from the oracle, as everywhere
else; tests/test_frontier_cases_cpu.py holds the model to the oracle's lists and prints, per case, the counts its `reaches` names.

The model restates the reference (src/planning/frontiers.cpp:25-85, 217-288) level by level: a level of a FIFO breadth-first
search is the concatenation, over the previous level in queue order, of each cell's newly visited neighbours in neighbour order.
It gives, per case: the classification (fr_classify), the widths of the 4-connected flood's levels, cells reached and levels in the
kernels' convention (counts[2], counts[3]), the touched frontier cells, and per frontier the 8-connected growth: its level widths
and the largest `tail - head` when eight queued cells are taken per step, as k_frontier_grow and k_frontier_grow2 take them.

No scipy, no random numbers: every map is written out by a few loops."""
import numpy as np

# ---- the kernels' constants (bl_frontiers.hip), restated
FR_T = 1024                 # threads of the one workgroup; a level up to here stays in registers
FR_B = 4                    # queue positions per thread in a batched level: FR_B * FR_T = 4096
FR_LQ = 4096                # next-level / growth-level entries mirrored in LDS
FR_CH = 8192                # slots of the claim table of fr_level_lds
FR_CH_PROBES = 128          # probes after which that table counts as full
FL_QMAX = 8192              # widest level k_frontier_flood keeps in LDS (FL_MAXB = 8 chunks of 1024)
FL_T = 1024
FR_RING = 1024              # growth queue entries mirrored in LDS by both grow kernels
FG_CELL_MAX = 16384         # frontier-class cells k_frontier_grow2's set holds
FG_SLOTS, FG_PAD, FG_DMAX = 32768, 128, 64
FR_HASH = 16384             # k_frontier_grow's visited set; a frontier may fill FR_HASH / 2 = 8192
FR_TOUCH_MAX = 16384        # touches the grow kernels keep
FR_CLS_LDS = 98304          # cells of the one-workgroup form
FL_MAX_SIDE = 16380         # longest side k_frontier_flood packs
M32 = 0xFFFFFFFF

MPC = np.float32(0.05)
CPM = np.float32(1.0 / np.float64(np.float32(0.05)))          # helpers.CPM_DEFAULT

_DX4, _DY4 = np.array([-1, 1, 0, 0]), np.array([0, 0, 1, -1])                             # frontiers.cpp:47-48
_DX8, _DY8 = np.array([-1, -1, -1, 1, 1, 1, 0, 0]), np.array([0, 1, -1, 0, 1, -1, 1, -1])   # :254-255


def frame(shape):
    h, w = shape
    return (np.float32(-w * 0.05 / 2), np.float32(-h * 0.05 / 2)), MPC


def pose_of_cell(shape, cell):
    """a point well inside `cell` (which may lie off the grid; the cast to int truncates towards zero, so a cell below zero is aimed
    at through its far half)"""
    origin, _ = frame(shape)
    return tuple(float(o) + (c + 0.5 if c >= 0 else c - 0.5) * 0.05 for o, c in zip(origin, cell))


def cell_of_pose(shape, xy):
    """global_position_to_grid_cell (grid_utils.hpp:33-38) on a float pose"""
    origin, _ = frame(shape)
    return tuple(int((float(np.float32(p)) - float(o)) * float(CPM)) for p, o in zip(xy, origin))


def classify(cells, robot):
    """fr_classify: 0 other, 1 free, 2 frontier-class, 3 the robot cell"""
    H, W = cells.shape
    v = cells.astype(np.int16)
    neg = v < 0
    nbneg = np.zeros((H, W), bool)                             # logOdds is 0 off the grid
    nbneg[:, 1:] |= neg[:, :-1]; nbneg[:, :-1] |= neg[:, 1:]
    nbneg[1:, :] |= neg[:-1, :]; nbneg[:-1, :] |= neg[1:, :]
    cls = np.zeros((H, W), np.uint8)
    cls[neg] = 1
    cls[(v <= 0) & (v >= -5) & nbneg] = 2
    if 0 <= robot[0] < W and 0 <= robot[1] < H:
        cls[robot[1], robot[0]] = 3
    return cls.ravel()


def _first_in_order(c):
    """the distinct values of c in the order of their first occurrence, and where that was"""
    _, first = np.unique(c, return_index=True)
    first.sort()
    return c[first], first


def fg_home(c):
    """k_frontier_grow2's home (fg_home), on an array of 32-bit words"""
    h = (np.asarray(c).astype(np.uint64) * np.uint64(2654435761)) & np.uint64(M32)
    h ^= h >> np.uint64(15)
    return (((h * np.uint64(0x85EBCA6B)) & np.uint64(M32)) >> np.uint64(17)).astype(np.int64)


class Model:
    def __init__(self, cells, robot, claim_tables=False):
        cells = np.ascontiguousarray(cells, dtype=np.int8)
        self.H, self.W = cells.shape
        self.robot = robot
        self.cls0 = classify(cells, robot)
        self.n_free = int((self.cls0 == 1).sum())
        self.n_frontier_class = int((self.cls0 == 2).sum())
        self._flood(claim_tables)
        self._sweep()

    # ---- the 4-connected flood (:47-82)
    def _flood(self, claim_tables):
        W, H = self.W, self.H
        cls = self.cls0.copy()
        x, y = np.array([self.robot[0]], np.int64), np.array([self.robot[1]], np.int64)
        base = 0
        self.flood_widths = [1]
        self.claim_tables = []                                 # per level of 1025..4096 cells: (width, distinct successors, verdict)
        tc = []
        while True:
            nx, ny = (x[:, None] + _DX4).ravel(), (y[:, None] + _DY4).ravel()          # key order: 4 p + n
            inb = (nx >= 0) & (nx < W) & (ny >= 0) & (ny < H)
            c = ny[inb] * W + nx[inb]
            k = cls[c]
            tc.append(c[k == 2])                               # touches, in key order
            new, _ = _first_in_order(c[k == 1])
            if claim_tables and FR_T < len(x) <= FR_B * FR_T:
                self.claim_tables.append((len(x), len(new), _claim_table_verdict(new)))
            if len(new) == 0:
                break
            cls[new] = 4
            base += len(x)
            x, y = new % W, new // W
            self.flood_widths.append(len(new))
        # the kernels' convention: counts[2] = queue positions, the robot's position 0 included; counts[3] = levels taken, the
        # robot's own and the last (which finds nothing new) included, i.e. the non-empty levels
        self.reached = int(sum(self.flood_widths))
        self.levels = len(self.flood_widths)
        tc = np.concatenate(tc)
        self.touched, _ = _first_in_order(tc)                  # touched frontier cells by first-touch key
        self.n_touched = len(self.touched)
        self._cls = cls

    # ---- frontiers in discovery order (:66-75), each grown FIFO over eight neighbours (:249-288)
    def _sweep(self):
        W, H = self.W, self.H
        cls = self._cls
        self.frontiers, self.grow_widths, self.backlog, self._children = [], [], [], []
        for seed in self.touched.tolist():
            if cls[seed] != 2:
                continue
            cls[seed] = 5
            cur = np.array([seed], np.int64)
            q, widths, children = [cur], [1], []
            while True:
                x, y = cur % W, cur // W
                nx, ny = (x[:, None] + _DX8).ravel(), (y[:, None] + _DY8).ravel()      # key order: 8 q + n
                idx = np.flatnonzero((nx >= 0) & (nx < W) & (ny >= 0) & (ny < H))
                c = ny[idx] * W + nx[idx]
                m = cls[c] == 2
                c, idx = c[m], idx[m]
                new, first = _first_in_order(c)
                children.append(np.bincount(idx[first] // 8, minlength=len(cur)))
                if len(new) == 0:
                    break
                cls[new] = 5
                q.append(new); widths.append(len(new))
                cur = new
            ch = np.concatenate(children)
            self.frontiers.append(np.concatenate(q))
            self.grow_widths.append(widths)
            self._children.append(ch)
            self.backlog.append(_largest_backlog(ch))
        del self._cls

    # ---- what the tests compare
    def lists(self, min_len):
        """the frontiers as the reference returns them: the length filter of :69 (size_t * float -> float, compared as double), cell
        corners as global points narrowed to float (grid_utils.hpp:14-19)"""
        (ox, oy), mpc = frame((self.H, self.W))
        out = []
        for f in self.frontiers:
            if not float(np.float32(len(f)) * mpc) >= min_len:
                continue
            xy = np.empty((len(f), 2), np.float32)
            xy[:, 0] = (float(ox) + (f % self.W).astype(np.float64) * float(mpc)).astype(np.float32)
            xy[:, 1] = (float(oy) + (f // self.W).astype(np.float64) * float(mpc)).astype(np.float32)
            out.append(xy)
        return out

    def stats(self):
        return self.reached, self.levels

    def widest_growth_level(self):
        return max((max(w) for w in self.grow_widths), default=0)

    def largest_backlog(self):
        return max(self.backlog, default=0)

    def largest_frontier(self):
        return max((len(f) for f in self.frontiers), default=0)

    def set_builds(self):
        """k_frontier_grow2's set of ALL frontier-class cells: does every cell find room within FG_DMAX slots of its home?  (Which
        slots end up taken does not depend on the order of the inserts; a cell's distance from home does, slightly.)"""
        cells = np.flatnonzero(self.cls0 == 2)
        if len(cells) > FG_CELL_MAX:
            return False
        tab = self._set_table(cells)
        return tab is not None

    def _set_table(self, cells):
        tab = np.full(FG_SLOTS + FG_PAD, -1, np.int64)
        for c, h in zip(cells.tolist(), fg_home(cells).tolist()):
            for d in range(FG_DMAX):
                if tab[h + d] == -1:
                    tab[h + d] = c
                    break
            else:
                return None
        return tab

    def probe_chains(self):
        """look-ups of k_frontier_grow2's growth that go past the home slot and the next (d >= 2): the neighbour is on the grid and both
        slots hold other cells"""
        cells = np.flatnonzero(self.cls0 == 2)
        tab = self._set_table(cells)
        n = 0
        for f in self.frontiers:
            x, y = f % self.W, f // self.W
            nx, ny = (x[:, None] + _DX8).ravel(), (y[:, None] + _DY8).ravel()
            inb = (nx >= 0) & (nx < self.W) & (ny >= 0) & (ny < self.H)
            c = ny[inb] * self.W + nx[inb]
            h = fg_home(c)
            v0, v1 = tab[h], tab[h + 1]
            n += int(((v0 != -1) & (v1 != -1) & (v0 != c) & (v1 != c)).sum())
        return n

    def take_duplicates(self):
        """lanes of one step of the growth (eight queued cells, eight neighbours each) that name a cell another lane of the step names
        too and that is not queued yet: FG_TAKE drops them with the first"""
        dup = 0
        for f, ch in zip(self.frontiers, self._children):
            if len(f) < 3:
                continue
            W, H = self.W, self.H
            where = np.full(W * H, -1, np.int64)               # queue position of a cell of this frontier
            where[f] = np.arange(len(f))
            x, y = f % W, f // W
            nx, ny = x[:, None] + _DX8, y[:, None] + _DY8
            inb = (nx >= 0) & (nx < W) & (ny >= 0) & (ny < H)
            npos = np.where(inb, where[np.where(inb, ny * W + nx, 0)], -1)
            tails = 1 + np.concatenate(([0], np.cumsum(ch)))           # tails[h]: the queue's tail once the cells below h are done
            head = 0
            while head < len(f):
                tail = int(tails[head])
                nb = min(tail - head, 8)
                names = npos[head:head + nb].ravel()
                names = names[names >= tail]
                dup += len(names) - len(np.unique(names))
                head += nb
        return dup

    def grow_v1_holds(self):
        """k_frontier_grow: every frontier within FR_HASH / 2 cells and every cell with room in the 64 slots behind its home"""
        for f in self.frontiers:
            if len(f) > FR_HASH // 2:
                return False
            tab = [-1] * FR_HASH
            homes = (((f.astype(np.uint64) * np.uint64(2654435761)) & np.uint64(M32)) >> np.uint64(18)).tolist()
            for c, h in zip(f.tolist(), homes):
                for l in range(64):
                    if tab[(h + l) & (FR_HASH - 1)] == -1:
                        tab[(h + l) & (FR_HASH - 1)] = c
                        break
                else:
                    return False
        return True

    def sweep_kernel(self, grow_v1=0):
        """bl_frontiers_debug_sweep_kernel: 0 the one-workgroup form, 3 k_frontier_grow2, 2 k_frontier_grow, 1 the one-workgroup sweep
        of the multi-launch form"""
        if self.W * self.H <= FR_CLS_LDS:
            return 0
        if self.n_touched > FR_TOUCH_MAX or self.W > 65535 or self.H > 32767:
            return 1
        if grow_v1 == 0 and self.set_builds():
            return 3
        return 2 if self.grow_v1_holds() else 1


def _largest_backlog(children):
    """the largest tail - head at the start of a step when min(tail - head, 8) queued cells are taken per step"""
    tails = 1 + np.concatenate(([0], np.cumsum(children)))
    head, worst = 0, 0
    n = len(children)
    while head < n:
        live = int(tails[head]) - head
        worst = max(worst, live)
        head += min(live, 8)
    return worst


def _claim_table_verdict(new):
    """fr_level_lds's claim table after a level has claimed the cells `new` (one entry per distinct cell, linear probing with wrap from
    a multiplicative home).  Which slots are taken does not depend on the order of the inserts: with no run of taken slots longer than
    FR_CH_PROBES no insert can probe that far ('fits'); more cells than slots cannot fit ('fills')."""
    if len(new) > FR_CH:
        return "fills"
    taken = bytearray(FR_CH)
    homes = (((new.astype(np.uint64) * np.uint64(2654435761)) & np.uint64(M32)) >> np.uint64(32 - 13)).tolist()
    for h in homes:
        while taken[h]:
            h = (h + 1) & (FR_CH - 1)
        taken[h] = 1
    t = np.frombuffer(bytes(taken) * 2, np.uint8)
    run = worst = 0
    for v in t.tolist():
        run = run + 1 if v else 0
        worst = max(worst, run)
    return "fits" if worst <= FR_CH_PROBES else "unknown"


# ---------------------------------------------------------------------------------------------------------------- the maps
def corridor_tree(W, H, L, value, field, centre=None):
    """Half-lengths L[0], L[1], ... drawn from the centre, alternately horizontal and vertical, each end carrying the next segment:
    all tips lie at one distance from the root, so whole flood levels are as wide as there are branches.  Returns cells, the root
    and the tips."""
    cells = np.full((H, W), field, np.int8)
    cx, cy = centre if centre else (W // 2, H // 2)
    ends = [(cx, cy)]
    for k, l in enumerate(L):
        nxt = []
        for (x, y) in ends:
            if k % 2 == 0:
                assert x - l >= 1 and x + l < W - 1
                cells[y, x - l:x + l + 1] = value
                nxt += [(x - l, y), (x + l, y)]
            else:
                assert y - l >= 1 and y + l < H - 1
                cells[y - l:y + l + 1, x] = value
                nxt += [(x, y - l), (x, y + l)]
        ends = nxt
    return cells, (cx, cy), ends


L260 = (64, 64, 32, 32, 16, 16, 8, 8, 4, 4, 2, 2)
L300 = (72, 72, 36, 36, 18, 18, 9, 9, 4, 4, 2, 2, 1, 1)
L520 = (128, 128, 64, 64, 32, 32, 16, 16, 8, 8, 4, 4, 2, 2)
L_A = (40, 40, 20, 20, 10, 10, 5, 5, 2, 2)                    # 6 673 cells
L_B = (32, 32, 16, 16, 8, 8, 4, 4, 2, 2)                      # 5 953 cells
L_C = (48, 48, 24, 24, 12, 12, 6, 6, 3, 3)                    # between 8 192 and 16 384 cells
L_TIPS = (96, 80, 48, 40, 24, 20, 12, 10, 6, 5, 3, 2)         # 4096 tips, each with room for three more free cells


def free_tree(W, H, L, field):
    def build():
        cells, root, _ = corridor_tree(W, H, L, -50, field)
        return cells
    return build, (W // 2, H // 2)


def frontier_tree(W, H, L):
    """the tree of -3 in a field of 60: only tree cells are frontier-class; one free robot cell beside the root"""
    def build():
        cells, (cx, cy), _ = corridor_tree(W, H, L, -3, 60)
        assert cells[cy - 1, cx] == 60
        cells[cy - 1, cx] = -50
        return cells
    return build, (W // 2, H // 2 - 1)


def tree_with_corridor():
    """the 520-cell tree and, on its topmost tip, a straight corridor: once the tree's widest levels are through (all tips lie at one
    distance), levels of one cell follow.  (A corridor from the root would add a cell to every level, and the levels of exactly
    FL_QMAX cells would be gone.)"""
    W, H = 520, 570
    cells, (cx, cy), tips = corridor_tree(W, H, L520, -50, 60, centre=(260, 260))
    tx, ty = max(tips, key=lambda t: (t[1], -t[0]))
    assert (cells[ty + 1:H - 8, tx - 1:tx + 2] == 60).all()
    cells[ty + 1:H - 8, tx] = -50
    return cells


def open_tips(W, H, L):
    """the tree, every tip opened to three more free cells: the last level of the tree has more distinct successors than itself"""
    def build():
        cells, (cx, cy), tips = corridor_tree(W, H, L, -50, 60, centre=(W // 2, H // 2))
        assert len(L) % 2 == 0                                 # the last segments are vertical: tips come as (lower, upper) pairs
        for i, (x, y) in enumerate(tips):
            s = -1 if i % 2 == 0 else 1
            for (ax, ay) in ((x - 1, y), (x + 1, y), (x, y + s)):
                assert cells[ay, ax] == 60
                cells[ay, ax] = -50
        return cells
    return build, (W // 2, H // 2)


def _block_value(x, y):
    return -((2 * x + 3 * y + (x * y) % 4) % 6)                # -5 .. 0, no two rows alike


def thick_block(W, H, side, robot_in_the_middle):
    """a free room, and next to it a block of side x side cells with values from -5 to 0: one thick frontier (a zero that has no
    negative neighbour is no frontier cell and leaves a hole).  The robot stands in the room -- the seed then lies on the block's
    edge -- or on one free cell in the block's middle."""
    x0, y0 = 24, 10
    def build():
        cells = np.full((H, W), 60, np.int8)
        cells[y0:y0 + side, 2:x0] = -50
        for y in range(y0, y0 + side):
            for x in range(x0, x0 + side):
                cells[y, x] = _block_value(x, y)
        if robot_in_the_middle:
            cells[y0 + side // 2, x0 + side // 2] = -50
        return cells
    return build, ((x0 + side // 2, y0 + side // 2) if robot_in_the_middle else (5, y0 + side // 2))


def small_room():
    cells = np.full((8, 11), -50, np.int8)
    cells[3:5, 4:7] = 0
    return cells


def large_room():
    cells = np.full((300, 400), -50, np.int8)
    cells[140:160, 190:210] = 0
    return cells


_STRIP = [-50] * 12 + [0] * 3 + [-50] * 6 + [-3] + [-50] * 8 + [0] * 7       # 37 cells


def strip(rows, transpose):
    def build():
        c = np.array([_STRIP, _STRIP[::-1]][:rows], np.int8)
        return np.ascontiguousarray(c.T if transpose else c)
    return build


def open_top(W, H):
    """free but for an unknown top row (one frontier that ends in the grid's last cell), a wall and a few weak cells"""
    def build():
        cells = np.full((H, W), -50, np.int8)
        cells[H - 1, :] = 0
        cells[H // 2, 10:W - 40] = 60
        cells[H // 3, 5:9] = (-5, -6, 0, -1)
        return cells
    return build


def three_lengths():
    """a free corridor under three runs of unknown cells: frontiers of 6, 7 and 8 cells.  At 0.05 m per cell and minFrontierLength
    0.35, the float product 7 * 0.05f is 0.349999994 (dropped), the double one 0.35000000000000003"""
    cells = np.full((5, 40), 60, np.int8)
    cells[2, 1:39] = -50
    cells[1, 2:8] = 0
    cells[1, 10:17] = 0
    cells[1, 19:27] = 0
    return cells


def lattice(W, H):
    """value 0 at even x and even y, every other cell -50: ceil(W/2) * ceil(H/2) frontiers of one cell, no two of them 8-connected"""
    cells = np.full((H, W), -50, np.int8)
    cells[0::2, 0::2] = 0
    return cells


LATTICES = [(9, 9), (9, 7), (15, 3), (3, 15), (11, 5), (7, 7)]         # (H, W)


# --------------------------------------------------------------------------------------------------------------- the cases
class Case:
    def __init__(self, name, build, robot, sweep, reaches, tags=(), claim_tables=False):
        self.name, self.build, self.robot, self.sweep, self.reaches, self.tags = name, build, robot, sweep, reaches, tuple(tags)
        self.claim_tables = claim_tables
        self._model = None

    def cells(self):
        return np.ascontiguousarray(self.build(), dtype=np.int8)

    def pose(self, shape):
        return pose_of_cell(shape, self.robot)

    def model(self):
        if self._model is None:
            self._model = Model(self.cells(), self.robot, self.claim_tables)
        return self._model

    def __repr__(self):
        return self.name


def _levels(m, lo, hi=None):
    return sum(1 for w in m.flood_widths if w > lo and (hi is None or w <= hi))


def _narrow_after_wide(m):
    """levels within FL_QMAX right behind one above it: fl_refill in mid-flood"""
    w = m.flood_widths
    return sum(1 for i in range(2, len(w)) if w[i - 1] > FL_QMAX >= w[i])


def _packed_behind_generic(m):
    """packed levels of 2 .. 8 chunks"""
    return _levels(m, FL_T, FL_QMAX)


CASES = []


def _add(*a, **k):
    CASES.append(Case(*a, **k))


# ---- the one-workgroup form (at most FR_CLS_LDS cells)
_b, _r = free_tree(260, 260, L260, 60)
_add("tree260_free", _b, _r, 0, lambda m: {"levels in (1024, 4096]: batched": _levels(m, FR_T, FR_B * FR_T),
                                           "widest level is 4096": int(max(m.flood_widths) == 4096)}, tags=("tree",))
_b, _r = free_tree(300, 300, L300, 60)
_add("tree300_free", _b, _r, 0, lambda m: {"levels above 4096: wide": _levels(m, FR_B * FR_T),
                                           "levels in (1024, 4096]: batched": _levels(m, FR_T, FR_B * FR_T)}, tags=("tree",))
for _n, _L, _S in (("tree260_rim", L260, 260), ("tree300_rim", L300, 300)):
    _b, _r = free_tree(_S, _S, _L, 0)
    _add(_n, _b, _r, 0, lambda m: {"a rim frontier of at least 10 000 cells": int(m.largest_frontier() >= 10000),
                                   "touched cells": m.n_touched,
                                   "levels above 1024 that touch it": _levels(m, FR_T)}, tags=("tree",))
_b, _r = frontier_tree(160, 160, L_A)
_add("fronttree_A", _b, _r, 0, lambda m: {"one frontier": int(len(m.frontiers) == 1),
                                          "widest growth level in (1024, 4096]": int(FR_T < m.widest_growth_level() <= FR_LQ)}, tags=("tree",))
_b, _r = frontier_tree(260, 260, L260)
_add("fronttree_260", _b, _r, 0, lambda m: {"one frontier": int(len(m.frontiers) == 1),
                                            "widest growth level above 4096: fq re-read": int(m.widest_growth_level() > FR_LQ)}, tags=("tree",))
for _mid in (False, True):
    _b, _r = thick_block(96, 64, 44, _mid)
    _add("block_small_" + ("middle" if _mid else "edge"), _b, _r, 0,
         lambda m: {"a frontier of at least 1600 cells (40 x 40)": int(m.largest_frontier() >= 1600),
                    "growth levels wider than 8 cells": sum(1 for w in m.grow_widths[0] if w > 8)}, tags=("block",))
for _name, _cell in (("left", (0, 4)), ("right", (10, 4)), ("bottom", (5, 0)), ("top", (5, 7)),
                     ("corner00", (0, 0)), ("corner10", (10, 0)), ("corner01", (0, 7)), ("corner11", (10, 7)),
                     ("off_left", (-1, 4)), ("off_right", (11, 4)), ("off_bottom", (5, -1)), ("off_top", (5, 8)),
                     ("off_corner00", (-1, -1)), ("off_corner11", (11, 8))):
    _off = _name.startswith("off_corner")
    _add("robot_" + _name, small_room, _cell, 0,
         (lambda m: {"nothing reached": int(m.reached == 1 and m.levels == 1)}) if _off else
         (lambda m: {"free cells reached": m.reached - 1, "frontiers": len(m.frontiers)}))
_add("grid_1x1", lambda: np.full((1, 1), -50, np.int8), (0, 0), 0, lambda m: {"one level": int(m.stats() == (1, 1))})
_add("grid_1xN", strip(1, False), (2, 0), 0, lambda m: {"frontiers": len(m.frontiers)})
_add("grid_Nx1", strip(1, True), (0, 2), 0, lambda m: {"frontiers": len(m.frontiers)})
_add("grid_2xN", strip(2, False), (2, 0), 0, lambda m: {"frontiers": len(m.frontiers)})
_add("grid_Nx2", strip(2, True), (0, 2), 0, lambda m: {"frontiers": len(m.frontiers)})
_add("lds_exactly_full", open_top(384, 256), (100, 100), 0,
     lambda m: {"cells == FR_CLS_LDS": int(m.W * m.H == FR_CLS_LDS), "the last cell is a frontier cell": int(m.cls0[-1] == 2 and len(m.frontiers) >= 1)})
_add("three_lengths", three_lengths, (1, 2), 0,
     lambda m: {"frontiers of 6, 7 and 8 cells": int(sorted(len(f) for f in m.frontiers) == [6, 7, 8]),
                "kept at 0.35": int(len(m.lists(0.35)) == 1 and 7 * 0.05 >= 0.35 > float(np.float32(7) * MPC))})

# ---- the multi-launch form
_add("first_multi_launch", open_top(247, 398), (100, 100), 3,
     lambda m: {"cells == FR_CLS_LDS + 2, no multiple of four": int(m.W * m.H == FR_CLS_LDS + 2 and (m.W * m.H) % 4 == 2),
                "the last cell is a frontier cell": int(m.cls0[-1] == 2)})
_add("tree520_corridor", tree_with_corridor, (260, 260), 3,
     lambda m: {"packed levels of 2 .. 8 chunks": _packed_behind_generic(m),
                "levels of exactly FL_QMAX cells": sum(1 for w in m.flood_widths if w == FL_QMAX),
                "levels above FL_QMAX: fl_level_generic in mid-flood": _levels(m, FL_QMAX),
                "a level within FL_QMAX behind one above it: fl_refill": _narrow_after_wide(m)}, tags=("tree",))
for _name, _cell in (("left", (-1, 150)), ("right", (400, 150)), ("bottom", (200, -1)), ("top", (200, 300))):
    _add("large_robot_off_" + _name, large_room, _cell, 3, lambda m: {"free cells reached": m.reached - 1, "frontiers": len(m.frontiers)})
for _n, _L in (("fronttree_big_A", L_A), ("fronttree_big_B", L_B)):
    _b, _r = frontier_tree(320, 320, _L)
    _add(_n, _b, _r, 3, lambda m: {"one frontier of at most 8191 cells": int(len(m.frontiers) == 1 and len(m.frontiers[0]) <= 8191),
                                   "backlog above FR_RING: the ring overtaken": int(m.largest_backlog() > FR_RING),
                                   "k_frontier_grow under BOTLAB_FRONTIER_GROW_V1": int(m.sweep_kernel(1) == 2)}, tags=("tree",))
_b, _r = frontier_tree(320, 330, L_C)
_add("fronttree_big_C", _b, _r, 3, lambda m: {"one frontier of 8192 .. 16 384 cells": int(len(m.frontiers) == 1 and FR_HASH // 2 <= len(m.frontiers[0]) <= FG_CELL_MAX),
                                              "handed down to the one-workgroup sweep under BOTLAB_FRONTIER_GROW_V1": int(m.sweep_kernel(1) == 1),
                                              "widest growth level above 1024": int(m.widest_growth_level() > FR_T)}, tags=("tree",))
for _mid in (False, True):
    _b, _r = thick_block(330, 320, 100, _mid)
    _add("block_large_" + ("middle" if _mid else "edge"), _b, _r, 3,
         lambda m: {"frontier-class cells within FG_CELL_MAX": int(0 < m.n_frontier_class <= FG_CELL_MAX),
                    "FG_TAKE: lanes of a step naming a cell again": m.take_duplicates(),
                    "look-ups past the home slot and the next (d >= 2)": m.probe_chains()}, tags=("block",))

# ---- a side above FL_MAX_SIDE: the flood through k_frontiers<FR_FLOOD_ONLY>
for _n, _t in (("long_side_x_tree300", False), ("long_side_y_tree300", True)):
    def _build(t=_t):
        cells, _, _ = corridor_tree(16384, 300, L300, -50, 60)
        return np.ascontiguousarray(cells.T) if t else cells
    _add(_n, _build, (150, 8192) if _t else (8192, 150), 3,
         lambda m: {"a side above FL_MAX_SIDE": int(max(m.W, m.H) > FL_MAX_SIDE),
                    "levels of 1025 .. 4096 cells whose claims fit the table: fr_level_lds<FR_B>": sum(1 for t in m.claim_tables if t[2] == "fits"),
                    "levels above 4096 behind them": _levels(m, FR_B * FR_T)}, tags=("tree",), claim_tables=True)
_b, _r = open_tips(16384, 322, L_TIPS)
_add("long_side_open_tips", _b, _r, 3,
     lambda m: {"a level of at most 4096 cells with more than FR_CH distinct successors: the table fills": sum(1 for t in m.claim_tables if t[2] == "fills"),
                "its width": max((t[0] for t in m.claim_tables if t[2] == "fills"), default=0),
                "its successors": max((t[1] for t in m.claim_tables if t[2] == "fills"), default=0)}, tags=("tree",), claim_tables=True)

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
