"""The closed loop of the obstacle tracks in the model (tests/obstacle_tracks_loop.py): a box the map does not know crosses the robot's
route at 0.7 cell per tick.  Three ways -- the map alone, the layer, the tracks with a horizon of ten updates -- and the figures of
each printed (DESIGN.md 4.24 records them).  No threshold is set on arrival ticks or on the steps inside the box with the tracks; what
is asserted is the scene itself (the speed was chosen so that the plain layer lets the robot into the box) and that the box keeps one
id while it is seen: on every tick on which the layer has a blob."""
import local_plan_model as lpm
import obstacle_tracks_loop as loop


def one_id_while_seen(ids):
    """ids: (tick, some track confirmed, ids holding a blob) per tick on which the layer has a blob.  On every such tick exactly one
    track holds a blob, and it is the same track throughout.  Returns its id."""
    assert ids and all(len(i) == 1 and i == ids[0][2] for _, _, i in ids), ids
    return ids[0][2][0]


def test_closed_loop_three_ways():
    out = {}
    for mode in ("map", "layer", "tracks"):
        r = loop.run_loop(mode)
        out[mode] = r
        all_ids = sorted(set(i for _, _, s in r["ids"] for i in s))
        print(f"{mode:7s} flags {int(r['recs'][-1]['flags'])} at tick {len(r['recs']) - 1}, {r['inside']} integration steps inside the box, "
              f"{r['blocked']} ticks stood still, ids {all_ids}, largest velocity error {r['verr']:.3f} cell per tick")
    assert out["map"]["inside"] >= 1 and out["layer"]["inside"] >= 1          # the scene: the layer alone does not keep the robot out
    assert all(int(out[m]["recs"][-1]["flags"]) == lpm.REACHED for m in out)
    kept = one_id_while_seen(out["tracks"]["ids"])
    print("the box keeps id", kept, "on every tick on which it is seen,", len(out["tracks"]["ids"]), "of them")
