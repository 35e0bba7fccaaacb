"""Measurement (recorded, not asserted): botlab_amd.LoopCloser.find_places, its descriptors + best pairs alone and the whole call
(DESIGN.md 4.34).

The two histories of tests/tools/loop_closure_probe.py -- 160 and 1024 scans of the world of tests/test_gpu_loop_closure.py -- at
stride 4 and stride 1.  One process, warmed up, then 7 repetitions; the host clock round each call, lastDeviceMs and its split from
events, whose first slot is k_pr_describe + k_pr_match.  Medians.  Writes a JSON file (default profiles/place_recognition_times.json).

    python tests/tools/place_probe.py [output.json]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

import botlab_amd as bl                       # noqa: E402
import test_gpu_loop_closure as lc            # noqa: E402
import loop_closure_probe as lcp              # noqa: E402

REPS = 7
PARAMS = {k: v for k, v in lcp.PARAMS.items() if k != "radius"}
PLACE = dict(bins_per_meter=4.0, place_max_range=8.0, dilate=1, min_key=16384, min_bits=8)


def _measure(ctx, history, like, n, stride):
    closer = bl.LoopCloser(1024, ctx=ctx)
    prm = dict(PARAMS, stride=stride, **PLACE)
    try:
        for _ in range(2):
            edges = closer.find_places(history, like, **prm)
        host, dev, split = [], [], []
        for _ in range(REPS):
            ctx.sync()
            t0 = time.perf_counter()
            closer.find_places(history, like, **prm)
            host.append((time.perf_counter() - t0) * 1e3)
            ms, ms4 = closer.lastDeviceMs(split=True)
            dev.append(ms)
            split.append(ms4)
        med = statistics.median
        places = closer.places()
        return dict(scans=n, stride=stride, queries=len(places), pairs_scored=int(sum(max(int(q) - prm["min_gap"], 0) for q in places["q"])),
                    candidates=len(closer.candidates()), kept=len(edges), repetitions=REPS, host_ms=med(host), device_ms=med(dev),
                    device_ms_describe_match=med(s[0] for s in split), device_ms_rays_fold=med(s[1] for s in split),
                    device_ms_match=med(s[2] for s in split), device_ms_records=med(s[3] for s in split),
                    all_device_ms_describe_match=[s[0] for s in split], all_device_ms=dev)
    finally:
        closer.close()


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "place_recognition_times.json")
    ctx = bl.default_context()
    rows = []
    for n in (160, 1024):
        history = lcp._history(ctx, n)
        like = bl.OccupancyGrid(lc.SIZE * lc.MPC, lc.SIZE * lc.MPC, lc.MPC, ctx=ctx)
        try:
            for stride in (4, 1):
                rows.append(_measure(ctx, history, like, n, stride))
                print(json.dumps({k: v for k, v in rows[-1].items() if not k.startswith("all_")}))
        finally:
            like.close(); history.close()
    with open(out, "w") as f:
        json.dump(dict(params={k: (float(v) if isinstance(v, float) else v) for k, v in dict(PARAMS, **PLACE).items()}, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
