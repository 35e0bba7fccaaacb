"""Time of pose-graph solves on the device and of the same graphs through the dense numpy solve on one host core:

    python tests/tools/pose_graph_probe.py [--out profiles/pose_graph_times.json] [--reps 7]

Graphs: two laps of a circle with odometry noise (tests/pose_graph_cases.loop_graph), (N, L) = (256, 8), (1024, 32), (4096, 64) with
one subset; (1024, 32) with 33 subsets (each loop edge alone, and all) and with 256 subsets (random masks).  Every shape is warmed up
once, then repeated; reported are the median and the least of bl_posegraph_last_device_ms (HIP events round the one launch), the
counters of subset 0, and the seconds of tests/pose_graph_model.dense_solve (np.linalg.solve of the normal equations with the same
step control; N = 4096 is a 12285 x 12285 system and is skipped unless --dense-large is given).  A measuring tool: it asserts nothing."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import botlab_amd as bl  # noqa: E402
import pose_graph_cases as pgc  # noqa: E402
import pose_graph_model as pgm  # noqa: E402


def measure(ctx, n, l, subsets, reps, dense):
    g, _ = pgc.loop_graph(n, l, seed=n, drift=0.002 if n < 4096 else 0.0005)
    if subsets == 1:
        masks = None
    elif subsets == l + 1:
        masks = np.zeros((subsets, (l + 31) // 32), np.uint32)
        for s in range(l):
            masks[s, s >> 5] = np.uint32(1) << np.uint32(s & 31)
        masks[l] = 0xffffffff
    else:
        masks = np.random.default_rng(1).integers(0, 1 << 32, (subsets, (l + 31) // 32), dtype=np.uint64).astype(np.uint32)
    pg = bl.PoseGraph(n, l, subsets, ctx=ctx)
    nodes = np.zeros(n, bl.POSE_DTYPE)
    nodes["x"], nodes["y"], nodes["theta"] = g.nodes[:, 0], g.nodes[:, 1], g.nodes[:, 2]
    e = bl.posegraph_edges(g.i, g.j, g.z, g.info)
    pg.set_nodes(nodes); pg.set_chain(e[:n - 1]); pg.set_loops(e[n - 1:])
    ms = []
    for rep in range(reps + 1):
        pg.solve(bl.posegraph_params(), masks)
        if rep:
            ms.append(pg.lastDeviceMs())
    r = pg.results()
    out = {"nodes": n, "loop_edges": l, "subsets": subsets, "reps": reps, "device_ms_median": statistics.median(ms), "device_ms_min": min(ms),
           "tries": int(r[0]["tries"]), "accepted": int(r[0]["accepted"]), "cg_iterations": int(r[0]["cg_iterations"]), "status": int(r[0]["status"]),
           "cost_before": float(r[0]["cost_before"]), "cost_after": float(r[0]["cost_after"]),
           "cg_iterations_max_over_subsets": int(r["cg_iterations"].max()), "tries_max_over_subsets": int(r["tries"].max())}
    pg.close()
    if dense:
        t = time.perf_counter()
        _, F, tries, accepted = pgm.dense_solve(g, pgm.DEFAULT, None if masks is None else masks[0])
        out.update({"dense_host_s": time.perf_counter() - t, "dense_cost_after": float(F), "dense_tries": tries, "dense_accepted": accepted})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_graph_times.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dense-large", action="store_true")
    a = ap.parse_args()
    os.environ.setdefault("OMP_NUM_THREADS", "1")
    ctx = bl.default_context()
    results = []
    for n, l, s in ((256, 8, 1), (1024, 32, 1), (4096, 64, 1), (1024, 32, 33), (1024, 32, 256)):
        results.append(measure(ctx, n, l, s, a.reps, dense=(s == 1 and (n < 4096 or a.dense_large))))
        print(json.dumps(results[-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tests/tools/pose_graph_probe.py", "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
