"""What the sampling local planner's tests share: parameter sets, the states of the mixed batch, the hand-built pillar world with its
pinned fall-back case, the closed loop of the model (computed once per process), and the comparison of everything the device hands
back with tests/mppi_model.py, byte for byte."""
import functools
import math

import numpy as np

import local_plan_model as lpm
import mppi_model as mm
import test_local_plan_model_cpu as cpu

F32 = np.float32
CPM = cpu.CPM

# the ragged 203 x 117 world: reversing allowed, all three weights in play
RAGGED = dict(v_min=-0.1, v_max=0.5, w_max=2.5, acc_v=3.0, acc_w=20.0, dt_sim=0.05, noise_v=0.25, noise_w=1.5, n_samples=65, horizon=6, n_sub=2,
              lam=64, w_field=7, w_heading=3, w_clear=2, seed=0x1234567887654321)


def ragged_state(world, tick=3, stream=5):
    return (cpu.cell_centre(world, 24, 54) + (F32(0.4),), F32(0.2), F32(-0.3), tick, stream)


def nominal(p, seed=2):
    """A nominal sequence with both signs in it, within the fixed-point range."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(-20000, 40000, p.T), rng.integers(-150000, 150000, p.T)], axis=1).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- the mixed batch
POCKET = dict(v_min=0.3, v_max=0.5, w_max=2.0, acc_v=0.0, acc_w=8.0, dt_sim=0.05, noise_v=0.25, noise_w=1.5, n_samples=65, horizon=6, n_sub=2,
              lam=64, w_field=1, w_heading=1, w_clear=1, seed=77)


def batch_states():
    """On cpu.pocket_world(): normal (in the corridor, facing the goal), REACHED, off the grid, on a wall, on an unreached cell,
    BLOCKED (the one-cell pocket at the corridor's far end).  (pose, v, w, tick, stream) each."""
    w = cpu.pocket_world()
    at = lambda x, y, th: cpu.cell_centre(w, x, y) + (F32(th),)
    return [(at(10, 15, math.pi), F32(0.4), F32(0.0), 1, 0), (at(5, 15, 2.0), F32(0.4), F32(0.1), 2, 1),
            ((F32(-1.5), at(10, 15, 0)[1], F32(0.0)), F32(0.4), F32(0.0), 3, 2), (at(3, 3, 0.0), F32(0.4), F32(0.0), 4, 3),
            (at(25, 25, 0.0), F32(0.4), F32(0.0), 5, 4), (at(15, 15, 0.0), F32(0.4), F32(0.0), 6, 5)]


BATCH_FLAGS = [0, mm.REACHED, mm.OFF_FIELD, mm.OFF_FIELD, mm.OFF_FIELD, mm.BLOCKED]


# ---------------------------------------------------------------------------------------------------------------- the pillar
PILLAR = dict(v_min=0.0, v_max=0.5, w_max=2.5, acc_v=0.0, acc_w=20.0, dt_sim=0.05, noise_v=0.25, noise_w=8.0, n_samples=128, horizon=8, n_sub=2,
              lam=4096, w_field=1, w_heading=0, w_clear=0)
PILLAR_START, PILLAR_GOAL = (12, 20), (34, 20)
PILLAR_SEED, PILLAR_TICK = 3, 7                              # test_mppi_model_cpu.test_fall_back_search pins these


@functools.lru_cache(maxsize=None)
def pillar_world():
    """A 47 x 41 room with a pillar one cell thick and three wide straight ahead of the start and the goal behind it: the ways round it are symmetric."""
    c = cpu.uniform_cells(47, 41)
    c[19:22, 20] = 100
    return cpu.make_world(c, cpu.ORIGIN, cpu.MPC, [PILLAR_GOAL], 0, cpu.SMALL_NAV)[0]


def pillar_state(world, tick):
    return (cpu.cell_centre(world, *PILLAR_START) + (F32(0.0),), F32(0.5), F32(0.0), tick, 0)


def pillar_nominal(p):
    """Full speed straight ahead: into the pillar."""
    return np.tile(np.array([[mm.q16(0.5), 0]], np.int32), (p.T, 1))


# ---------------------------------------------------------------------------------------------------------------- the closed loop
LOOP = dict(v_min=0.0, v_max=0.5, w_max=2.5, acc_v=2.0, acc_w=12.0, dt_sim=0.05, noise_v=0.25, noise_w=1.5, n_samples=1024, horizon=10, n_sub=2,
            lam=64, w_field=16, w_heading=1, w_clear=1, seed=1)
LOOP_CAP = 148                                               # test_local_plan_model_cpu's cap for this world, start and goal


def run_loop(world, p, pose, cap, step, stream=0):
    """Ticks of (plan, drive, advance) from `pose` at rest; step(pose, v, w, tick, stream, seq) -> (RESULT record, seq_out).  Returns the
    records, the sequences out and the cells passed through."""
    v, w = F32(0), F32(0)
    seq = np.zeros((p.T, 2), np.int32)
    recs, seqs, cells = [], [], []
    for tick in range(cap):
        r, so = step(pose, v, w, tick, stream, seq)
        recs.append(r)
        seqs.append(np.array(so, np.int32))
        flags = int(r["flags"])
        if flags & ~mm.FELL_BACK:
            break
        v, w = F32(r["trans_v"]), F32(r["angular_v"])
        for q in mm.drive(pose, so[0], p):
            cells.append(world.cell(q[0], q[1]))
            pose = q
        seq = mm.advance(np.array(so, np.int32), flags)
    return recs, seqs, cells


@functools.lru_cache(maxsize=None)
def model_loop():
    """The model's closed loop on test_local_plan_model_cpu's loop world, once per process."""
    world = cpu.loop_world()[0]
    p = mm.Params(**LOOP)
    return run_loop(world, p, cpu.loop_start(world), LOOP_CAP, lambda q, v, w, tick, stream, seq: mm.plan(world, p, q, v, w, tick, stream, seq)[:2])


# ---------------------------------------------------------------------------------------------------------------- device against model
RECORD_FIELDS = ("trans_v", "angular_v", "index_best", "n_admissible", "cost_best", "cost_out", "weight_sum", "weight_sq_sum", "flags")


def same_record(got, exp):
    return all(got[k].tobytes() == exp[k].tobytes() for k in RECORD_FIELDS)


def set_params(mp, p):
    mp.set_params(p.v_min, p.v_max, p.w_max, p.acc_v, p.acc_w, p.dt_sim, p.noise_v, p.noise_w, p.K, p.T, p.n_sub, p.lam, p.w_field, p.w_heading,
                  p.w_clear, p.seed)


def dev_state(bl, s, utime=99):
    pose, v, w, tick, stream = s
    return (bl.make_pose(pose[0], pose[1], pose[2], utime=utime), F32(v), F32(w), tick, stream)


def compare_samples(bl, mp, nf, world, p, s, u_in=None, tracker=None, moving=None, slots=None, m=None):
    """bl_mppi_debug_samples of one state against the model: all K costs, first hits and sequences.  Returns the model's three."""
    set_params(mp, p)
    costs, fh, seqs = mp.debug_samples(nf, dev_state(bl, s), u_in, tracker, moving)
    assert mp.debugPath() == (0 if p.staged(CPM) else 1)
    ec, ef, es = mm.debug_samples(world, p, s[0], s[1], s[2], s[3], s[4], u_in, slots, m)
    assert seqs.shape == es.shape
    bad = np.flatnonzero((seqs != es).any(axis=(1, 2)))
    assert len(bad) == 0, ("sequences", len(bad), int(bad[0]), seqs[bad[0]].tolist(), es[bad[0]].tolist())
    bad = np.flatnonzero(costs != ec)
    assert len(bad) == 0, ("costs", len(bad), int(bad[0]), int(costs[bad[0]]), int(ec[bad[0]]))
    bad = np.flatnonzero(fh != ef)
    assert len(bad) == 0, ("first hits", len(bad), int(bad[0]), int(fh[bad[0]]), int(ef[bad[0]]))
    return ec, ef, es


def compare_plan(bl, mp, nf, world, p, states, u_in=None, tracker=None, moving=None, slots=None, m=None):
    """bl_mppi_plan of `states` in one call against the model, and each state planned alone against the batch.  u_in [n, T, 2] or
    None.  Returns the model's (record, seq_out) per state."""
    set_params(mp, p)
    dev = [dev_state(bl, s) for s in states]
    got, seq = mp.plan(nf, dev, u_in, tracker, moving)
    out = []
    for i, s in enumerate(states):
        exp, eso, _ = mm.plan(world, p, s[0], s[1], s[2], s[3], s[4], None if u_in is None else u_in[i], slots, m)
        assert same_record(got[i], exp), (i, got[i], exp)
        assert seq[i].tobytes() == eso.tobytes(), (i, seq[i].tolist(), eso.tolist())
        if len(states) > 1:
            one, one_seq = mp.plan(nf, [dev[i]], None if u_in is None else u_in[i:i + 1], tracker, moving)
            assert one.tobytes() == got[i:i + 1].tobytes() and one_seq.tobytes() == seq[i:i + 1].tobytes(), i
        out.append((exp, eso))
    return out
