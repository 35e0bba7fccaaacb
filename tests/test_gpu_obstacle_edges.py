"""The scripts of tests/obstacle_edge_cases.py on the device beside the models, value for value after every step: the launch shapes
of bl_obstracks.hip and bl_obslayer.hip that the scripts of the definition do not reach (tests/test_obstacle_edge_cases_cpu.py shows
from the models that these do)."""
import numpy as np
import pytest

import obstacle_edge_cases as ec
import test_gpu_obstacle_layer as glayer
import test_gpu_obstacle_tracks as gtracks

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", [n for n, _ in ec.TRACK_CASES])
def test_tracks_script_equals_the_model(gpu_ctx, name):
    script, model, _ = ec.tracks_model_of(name)
    gtracks.run_both(gpu_ctx, script, model)


@pytest.mark.parametrize("name", [n for n, _ in ec.LAYER_CASES])
def test_layer_script_equals_the_model(gpu_ctx, name):
    script, model, _ = ec.layer_model_of(name)
    assert glayer.run_both(gpu_ctx, script) is not None
    if name == "far_poses":
        return
    dev = glayer.Device(gpu_ctx, script)                   # the capped lists, from the uploaded state
    try:
        assert dev.step(script.steps[0]) == "ok"
        live = model[0][1]["live"]
        for cap in ec.caps_of(script, live):
            got = dev.layer.live_cells(cap=cap)
            assert got.shape == live[:cap].shape and np.array_equal(got, live[:cap]), (name, cap)
        assert np.array_equal(dev.layer.live_cells(), live)
    finally:
        dev.close()
