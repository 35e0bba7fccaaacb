"""The sampling local planner's edges on the GPU against tests/mppi_model.py, byte for byte: rollouts that leave each side of the grid,
the pinned fall-back, ties of (cost, k), the two ends of lambda, the Philox counter words, and the refusals."""
import math

import numpy as np
import pytest

import botlab_amd as bl
from botlab_amd import _capi
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


FAST = dict(mc.RAGGED, v_min=0.0, v_max=1.0, acc_v=10.0, acc_w=30.0, w_max=3.0, horizon=10, n_sub=4, n_samples=257, noise_v=0.5, noise_w=3.0)


@pytest.mark.parametrize("name,cell,th", [("left", (2, 18), math.pi), ("right", (38, 18), 0.0), ("bottom", (20, 2), -math.pi / 2), ("top", (20, 34), math.pi / 2)])
def test_rollouts_leave_each_side_of_the_grid(gpu_ctx, mp, name, cell, th):
    world = cpu.open_world()
    p = mm.Params(**FAST)
    s = (cpu.cell_centre(world, *cell) + (F32(th),), F32(0.8), F32(0.0), 1, 2)
    u = None                                                                          # the robot arrives at 0.8 m/s and can only brake so fast
    xs, ys, ths, cx, cy, inside = mm.rollouts(world, p, s[0], mm.sample_seqs(p, s[1], s[2], s[3], s[4], u))
    assert (~inside).any(axis=1).sum() > 10 and inside.all(axis=1).sum() > 10, name      # some leave, some stay
    costs, _, _ = mc.compare_samples(bl, mp, _device(world, gpu_ctx), world, p, s, u)
    assert (costs[(~inside).any(axis=1)] == mm.COST_NONE).all()
    mc.compare_plan(bl, mp, _device(world, gpu_ctx), world, p, [s])


def test_the_pinned_fall_back(gpu_ctx, mp):
    world = mc.pillar_world()
    p = mm.Params(**dict(mc.PILLAR, seed=mc.PILLAR_SEED))
    s = mc.pillar_state(world, mc.PILLAR_TICK)
    out = mc.compare_plan(bl, mp, _device(world, gpu_ctx), world, p, [s], mc.pillar_nominal(p)[None])
    r, so = out[0]
    assert int(r["flags"]) == mm.FELL_BACK and int(r["cost_out"]) == int(r["cost_best"]) and int(r["index_best"]) > 1 and so.any()


def test_ties_go_to_the_lowest_sample(gpu_ctx, mp):
    """v_min = v_max = 0: every sample turns on the spot, on one cell, at one cost."""
    world = cpu.uniform_world()
    p = mm.Params(**dict(mc.RAGGED, v_min=0.0, v_max=0.0, w_heading=0, n_samples=300))
    s = (cpu.cell_centre(world, 20, 23) + (F32(0.3),), F32(0.0), F32(0.0), 0, 0)
    costs, _, seqs = mc.compare_samples(bl, mp, _device(world, gpu_ctx), world, p, s)
    assert len(set(costs.tolist())) == 1 and costs[0] != mm.COST_NONE and len({q.tobytes() for q in seqs}) > 100
    r, _ = mc.compare_plan(bl, mp, _device(world, gpu_ctx), world, p, [s])[0]
    assert int(r["index_best"]) == 0 and int(r["n_admissible"]) == 300 and int(r["weight_sum"]) == 300 << 24


def test_lambda_one_leaves_nearly_every_weight_zero(gpu_ctx, mp):
    world = cpu.ragged_world()
    p = mm.Params(**dict(mc.RAGGED, lam=1, w_field=65535, n_samples=257))
    r, _ = mc.compare_plan(bl, mp, _device(world, gpu_ctx), world, p, [mc.ragged_state(world)], mc.nominal(p)[None])[0]
    assert int(r["n_admissible"]) > 100 and int(r["weight_sum"]) < 4 << 24
    print("lambda 1: admissible", int(r["n_admissible"]), "weight sum / 2^24 =", int(r["weight_sum"]) / 2 ** 24)


def test_largest_lambda_and_sample_count_with_a_negative_numerator(gpu_ctx, mp):
    """lambda 2^30, K 16384, the nominal at -31 rad/s: every weight is 2^24, N is near -2^59 and the division floors a negative."""
    world = cpu.uniform_world()
    p = mm.Params(**dict(mc.RAGGED, v_min=0.0, v_max=0.0, w_max=31.0, acc_w=300.0, noise_w=1.0, lam=1 << 30, n_samples=16384, horizon=2, n_sub=1, w_field=1,
                         w_heading=1, w_clear=0))
    assert p.ok()
    s = (cpu.cell_centre(world, 20, 23) + (F32(0.3),), F32(0.0), F32(-31.0), 9, 9)
    u = np.tile(np.array([[0, mm.q16(-31.0)]], np.int32), (p.T, 1))
    r, so = mc.compare_plan(bl, mp, _device(world, gpu_ctx), world, p, [s], u[None])[0]
    assert int(r["weight_sum"]) == 16384 << 24 and int(r["weight_sq_sum"]) == 16384 << 48 and int(r["n_admissible"]) == 16384
    assert -mm.q16(31.0) <= so[0, 1] < -mm.q16(30.0)
    mc.compare_samples(bl, mp, _device(world, gpu_ctx), world, p, s, u)


def test_tick_and_stream_each_change_the_draw(gpu_ctx, mp):
    world = cpu.ragged_world()
    p = mm.Params(**mc.RAGGED)
    nf = _device(world, gpu_ctx)
    seen = set()
    for tick, stream in ((3, 5), (4, 5), (3, 6), (5, 3)):
        _, _, seqs = mc.compare_samples(bl, mp, nf, world, p, mc.ragged_state(world, tick, stream))
        seen.add(seqs[2:].tobytes())
    assert len(seen) == 4
    q = mm.Params(**dict(mc.RAGGED, seed=mc.RAGGED["seed"] ^ (1 << 32)))             # the seed's high word is a key word of its own
    _, _, seqs = mc.compare_samples(bl, mp, nf, world, q, mc.ragged_state(world, 3, 5))
    assert seqs[2:].tobytes() not in seen


def test_every_refusal_leaves_the_handle_as_it_was(gpu_ctx, mp):
    world = cpu.ragged_world()
    nf = _device(world, gpu_ctx)
    p = mm.Params(**mc.RAGGED)
    s = mc.ragged_state(world)
    before = mc.compare_plan(bl, mp, nf, world, p, [s])[0]
    good = dict(v_min=p.v_min, v_max=p.v_max, w_max=p.w_max, acc_v=p.acc_v, acc_w=p.acc_w, dt_sim=p.dt_sim, noise_v=p.noise_v, noise_w=p.noise_w,
                n_samples=p.K, horizon=p.T, n_sub=p.n_sub, lam=p.lam, w_field=p.w_field, w_heading=p.w_heading, w_clear=p.w_clear, seed=p.seed)
    bads = [dict(v_min=0.6), dict(w_max=-0.1), dict(dt_sim=0.0), dict(acc_v=float("nan")), dict(v_max=float("inf")), dict(noise_v=-0.1), dict(noise_w=-1.0),
            dict(acc_w=-1.0), dict(w_max=32.0), dict(noise_w=40.0), dict(acc_v=400.0), dict(n_samples=0), dict(n_samples=16385), dict(horizon=0), dict(horizon=65),
            dict(n_sub=0), dict(n_sub=17), dict(horizon=32, n_sub=8), dict(lam=0), dict(lam=(1 << 30) + 1), dict(w_field=65536), dict(w_clear=-1)]
    for bad in bads:
        assert not mm.Params(**dict(mc.RAGGED, **bad)).ok(), bad
        with pytest.raises(Exception):
            mp.set_params(**dict(good, **bad))
    mc.set_params(mp, p)
    dev = mc.dev_state(bl, s)
    nan_pose = bl.make_pose(float("nan"), 0.0, 0.0)
    for state in ((nan_pose, 0.0, 0.0, 0, 0), (dev[0], 32.0, 0.0, 0, 0), (dev[0], 0.0, -32.0, 0, 0), (bl.make_pose(0.0, 0.0, 70000.0), 0.0, 0.0, 0, 0)):
        with pytest.raises(Exception):
            mp.plan(nf, [state])
    assert not mm.state_ok(s[0], 32.0, 0.0) and mm.state_ok(s[0], 31.99, 0.0)
    with pytest.raises(Exception):                                                   # moving parameters without a tracker
        _one_sided(mp, nf, dev)
    skip = mm.Params(**dict(mc.RAGGED, v_max=1.5))                                    # a step of 0.075 m skips a cell of 0.05 m
    assert skip.ok() and skip.can_skip_a_cell(world.mpc)
    mc.set_params(mp, skip)
    with pytest.raises(Exception):
        mp.plan(nf, [dev])
    mc.set_params(mp, p)
    with pytest.raises(Exception):
        mp.rollout(nf, dev, np.full((p.T, 2), 1 << 21, np.int32))
    after = mc.compare_plan(bl, mp, nf, world, p, [s])[0]
    assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes()


def _one_sided(mp, nf, dev):
    """bl_mppi_plan with moving parameters and no tracker."""
    import ctypes as C
    s = (_capi.MppiState * 1)(mp._state(dev))
    out, seq = np.zeros(1, bl.MPPI_RESULT_DTYPE), np.zeros((mp.params.horizon, 2), np.int32)
    m = _capi.LocalPlanMoving(2, 0, 0, 0)
    _capi.check(mp.ctx.lib.bl_mppi_plan(mp.h, nf.h, None, C.byref(m), s, 1, None, seq.ctypes.data, out.ctypes.data))
