"""The sampling local planner's moving rule on the GPU against tests/mppi_model.py, byte for byte: a box that refuses samples, every
sample's first hit, a box over the pose's own cell, and the equality with the static call when no slot is used.  Tracks are placed by
bl_obstracks_upload."""
import numpy as np
import pytest

import botlab_amd as bl
import local_plan_moving_model as lmm
import mppi_cases as mc
import mppi_model as mm
import obstacle_tracks_model as tm
import test_mppi_model_cpu as cpu_m
from test_gpu_local_plan import _device

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(gpu_ctx):
    world = cpu_m.moving_case()[0]
    layer = bl.ObstacleLayer(world.w, world.h, ttl_scans=3, min_hits=1, ctx=gpu_ctx)
    tr = bl.ObstacleTracker(layer, **dict(tm.BASE, max_cells=9))
    mp = bl.MppiPlanner(gpu_ctx)
    yield mp, tr
    mp.close()
    tr.close()
    layer.close()


def _upload(tr, slots):
    tr.upload(slots, 0, int(slots["id"].max()) + 1, 1)


def test_a_crossing_box_refuses_samples_and_first_hits_equal_the_model(gpu_ctx, env):
    mp, tr = env
    world, p, s, slots, m = cpu_m.moving_case()
    nf = _device(world, gpu_ctx)
    _upload(tr, slots)
    moving = (m.q, m.margin, m.lead)
    costs, fh, _ = mc.compare_samples(bl, mp, nf, world, p, s, None, tr, moving, slots, m)
    assert 10 < np.count_nonzero(fh) < p.K - 10 and (costs[fh > 0] == mm.COST_NONE).all()
    r, _ = mc.compare_plan(bl, mp, nf, world, p, [s], None, tr, moving, slots, m)[0]
    plain, _ = mc.compare_plan(bl, mp, nf, world, p, [s])[0]
    assert r.tobytes() != plain.tobytes()
    u = mc.nominal(p)                                                                # a warm start, and two states in one call
    s2 = (s[0], s[1], s[2], s[3] + 1, s[4])
    mc.compare_plan(bl, mp, nf, world, p, [s, s2], np.stack([u, u]), tr, moving, slots, m)


def test_a_box_over_the_pose_is_blocked_not_off_field(gpu_ctx, env):
    mp, tr = env
    world, p, s, _, m = cpu_m.moving_case()
    over = lmm.slot_table([lmm.make_slot(3, 15, 18, 25, 28)])
    _upload(tr, over)
    r, so = mc.compare_plan(bl, mp, _device(world, gpu_ctx), world, p, [s], None, tr, (m.q, m.margin, m.lead), over, m)[0]
    assert int(r["flags"]) == mm.BLOCKED and int(r["n_admissible"]) == 0 and not so.any()
    _, fh, _ = mc.compare_samples(bl, mp, _device(world, gpu_ctx), world, p, s, None, tr, (m.q, m.margin, m.lead), over, m)
    assert (fh == 1).all()


def test_no_used_slot_is_the_static_call_byte_for_byte(gpu_ctx, env):
    mp, tr = env
    world, p, s, _, m = cpu_m.moving_case()
    nf = _device(world, gpu_ctx)
    unused = lmm.slot_table([lmm.make_slot(1, 26, 18, 28, 22, vx=-100, vy=60, flags=tm.CONFIRMED | tm.MOVING),
                             lmm.make_slot(2, 18, 20, 22, 26, flags=tm.MOVING | tm.MATCHED), lmm.make_slot(4, 19, 22, 21, 24, flags=tm.CONFIRMED | tm.BORN)])
    assert not lmm.used_slots(unused)
    _upload(tr, unused)
    mc.set_params(mp, p)
    dev = [mc.dev_state(bl, s)]
    u = mc.nominal(p)[None]
    got, seq = mp.plan(nf, dev, u, tr, (m.q, m.margin, m.lead))
    plain, pseq = mp.plan(nf, dev, u)
    assert got.tobytes() == plain.tobytes() and seq.tobytes() == pseq.tobytes() and int(got[0]["flags"]) in (0, mm.FELL_BACK)
    c1, f1, q1 = mp.debug_samples(nf, dev[0], u[0], tr, (m.q, m.margin, m.lead))
    c0, f0, q0 = mp.debug_samples(nf, dev[0], u[0])
    assert c1.tobytes() == c0.tobytes() and q1.tobytes() == q0.tobytes() and not f1.any() and not f0.any()
