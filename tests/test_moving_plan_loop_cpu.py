"""The closed loop of the local planner's moving rule in the model (tests/moving_plan_loop.py): DESIGN.md 4.24's room and crossing box,
the field over the static composition, the commands from command_moving.  No arrival tick is fixed; what is asserted is that the loop
arrives, that the prediction does no worse than no prediction (the steps inside the true box against the layer's loop, computed
here), and -- from the definition, not as a measurement -- that with a box that stands still the records are the layer loop's."""
import local_plan_model as lpm
import local_plan_moving_model as lmm
import moving_plan_loop as ml
import obstacle_tracks_loop as tl


def test_the_loop_arrives_and_does_no_worse_than_the_layer():
    layer = ml.layer_run()
    r = ml.run_loop()
    print(f"moving  flags {int(r['recs'][-1]['flags'])} at tick {len(r['recs']) - 1}, {r['inside']} integration steps inside the box, {r['blocked']} ticks "
          f"stood still, a moving box refused candidates on {sum(1 for n in r['refused'] if n)} ticks, passed {r['crossed']} the box")
    print(f"layer   flags {int(layer['recs'][-1]['flags'])} at tick {len(layer['recs']) - 1}, {layer['inside']} integration steps inside the box")
    assert int(r["recs"][-1]["flags"]) == lpm.REACHED and len(r["recs"]) <= tl.TICKS
    assert r["inside"] <= layer["inside"]
    assert any(r["refused"])                                          # the rule was at work


def test_a_box_that_stands_still_is_the_layer_loop_byte_for_byte():
    """Without a MOVING track the static composition is the layer's and no slot is used: the records are the layer loop's by the
    definition.  The scene's own tracker does flag the standing box MOVING on some ticks -- its visible part grows as the robot comes
    nearer, which moves the centroid --, so the run that shows the definition's consequence sets min_speed to its limit, which no
    velocity here reaches; the run with the scene's parameters is compared as well and its MOVING ticks are printed."""
    layer = ml.layer_run(0.0)
    for name, tracks in (("min_speed 1023", dict(tl.TRACKS, min_speed=1023)), ("the scene's parameters", None)):
        used = []
        r = ml.run_loop(speed=0.0, tracks=tracks, on_tick=lambda tick, l, t, scan, pose, composed, world: used.append(len(lmm.used_slots(t.slots))))
        assert len(used) == len(r["recs"]) and (tracks is None or not any(used))
        assert len(r["recs"]) == len(layer["recs"]) and all(a.tobytes() == b.tobytes() for a, b in zip(r["recs"], layer["recs"]))
        assert (r["inside"], r["blocked"]) == (layer["inside"], layer["blocked"])
        print(f"standing box, {name}: {len(r['recs'])} records equal the layer loop's; a used slot on {sum(1 for u in used if u)} ticks")
