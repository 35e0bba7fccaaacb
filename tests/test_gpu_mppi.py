"""The sampling local planner on the GPU (bl_mppi_*, botlab_amd/csrc/bl_mppi.hip) against its model (tests/mppi_model.py): every
sample's cost and sequence, the results and the sequences out, byte for byte and with nothing left out, on the sample counts and
horizons at which the kernels take another path; the model's closed loop tick for tick through advance()."""
import numpy as np
import pytest

import botlab_amd as bl
import mppi_cases as mc
import mppi_model as mm
import test_local_plan_model_cpu as cpu
from test_gpu_local_plan import _device

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def mp(gpu_ctx):
    p = bl.MppiPlanner(gpu_ctx)
    yield p
    p.close()


def test_weight_table_is_the_models(mp):
    assert mp.weightTable().tolist() == mm.weight_table()


@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 257, 1024])
def test_samples_equal_the_model_at_every_count(gpu_ctx, mp, K):
    world = cpu.ragged_world()
    p = mm.Params(**dict(mc.RAGGED, n_samples=K))
    costs, _, seqs = mc.compare_samples(bl, mp, _device(world, gpu_ctx), world, p, mc.ragged_state(world), mc.nominal(p))
    assert (costs != mm.COST_NONE).any()
    assert (seqs[0] == mm.clamp_seq(p, mc.nominal(p), 0.2, -0.3)).all() and (K < 2 or (seqs[1, -1] == 0).all())
    got = mc.compare_plan(bl, mp, _device(world, gpu_ctx), world, p, [mc.ragged_state(world)], mc.nominal(p)[None])
    assert int(got[0][0]["flags"]) in (0, mm.FELL_BACK)


@pytest.mark.parametrize("T,n_sub,v_max,staged", [(1, 1, 0.5, True), (17, 15, 0.1, True), (51, 5, 0.5, False), (37, 4, 0.5, True), (38, 4, 0.5, False)])
def test_horizons_and_both_sides_of_the_window_rule(gpu_ctx, mp, T, n_sub, v_max, staged):
    """1 and 255 integration steps; 148 and 152 steps at 0.5 m/s lie on either side of BL_LOCALPLAN_WINDOW_BYTES."""
    world = cpu.ragged_world()
    p = mm.Params(**dict(mc.RAGGED, horizon=T, n_sub=n_sub, v_max=v_max, acc_w=2.0, acc_v=0.3))
    assert p.ok() and p.staged(mc.CPM) == staged
    s = mc.ragged_state(world)
    mc.compare_samples(bl, mp, _device(world, gpu_ctx), world, p, s, mc.nominal(p))
    mc.compare_plan(bl, mp, _device(world, gpu_ctx), world, p, [s], mc.nominal(p)[None])
    poses = mp.rollout(_device(world, gpu_ctx), mc.dev_state(bl, s), mc.nominal(p) // 4)
    xs, ys, ths = mm.poses(p, s[0], (mc.nominal(p) // 4)[None])
    assert (poses["utime"] == 99).all()
    assert poses["x"].tobytes() == xs[0].tobytes() and poses["y"].tobytes() == ys[0].tobytes() and poses["theta"].tobytes() == ths[0].tobytes()


def test_batches_equal_the_model_and_each_state_alone(gpu_ctx, mp):
    world = cpu.pocket_world()
    p = mm.Params(**mc.POCKET)
    nf = _device(world, gpu_ctx)
    mc.set_params(mp, p)
    got, seq = mp.plan(nf, [])                                                       # n = 0
    assert len(got) == 0 and len(seq) == 0
    states = mc.batch_states()
    one = mc.compare_plan(bl, mp, nf, world, p, states[:1])                           # n = 1, no nominal
    assert int(one[0][0]["flags"]) in (0, mm.FELL_BACK) and int(one[0][0]["n_admissible"]) > 0
    u = np.stack([mc.nominal(p, seed=k) for k in range(len(states))])
    out = mc.compare_plan(bl, mp, nf, world, p, states, u)
    assert [int(r["flags"]) & ~mm.FELL_BACK for r, _ in out] == mc.BATCH_FLAGS
    for (r, so), f in zip(out[1:], mc.BATCH_FLAGS[1:]):
        assert not so.any() and int(r["index_best"]) == -1 and float(r["trans_v"]) == 0.0 and int(r["cost_out"]) == (0 if f == mm.REACHED else mm.COST_NONE)
    for k in (4, 5):                                                                  # the debug call rolls out whatever the flags
        mc.compare_samples(bl, mp, nf, world, p, states[k], u[k])


def test_closed_loop_tick_for_tick_through_advance(gpu_ctx):
    world = cpu.loop_world()[0]
    nf = _device(world, gpu_ctx)
    p = mm.Params(**mc.LOOP)
    recs, seqs, cells = mc.model_loop()
    assert int(recs[-1]["flags"]) == mm.REACHED
    mp = bl.MppiPlanner(gpu_ctx)
    try:
        mc.set_params(mp, p)
        tick = [0]

        def step(pose, v, w, t, stream, seq):
            assert mp.tick == t and mp.seq.tobytes() == np.asarray(seq, np.int32).tobytes()
            mp.command(nf, bl.make_pose(pose[0], pose[1], pose[2], utime=t), v, w, stream)
            r, so = mp.last.copy(), mp.seq.copy()
            assert mc.same_record(r, recs[t]) and so.tobytes() == seqs[t].tobytes(), (t, r, recs[t])
            mp.advance()
            tick[0] += 1
            return r, so

        got, _, dcells = mc.run_loop(world, p, cpu.loop_start(world), mc.LOOP_CAP, step)
        assert len(got) == len(recs) and dcells == cells
        print("closed loop on the device: %d ticks, %.3f ms of kernels in the last" % (len(got) - 1, mp.lastDeviceMs()))
    finally:
        mp.close()
