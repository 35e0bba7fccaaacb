"""Generates tests/golden/astar_edge_cases.json: start / goal pairs on the border worlds of tests/astar_edge_cases.py (ring(61, 37, 6) and
a ring of more than 524 288 cells), every one starting or ending on a corner cell of the grid or turning a corner.  With the
reference's cost function and no open-list de-duplication a pair a few cells off one row costs 1e5 .. 1e8 pops, so the candidates run
through the CPU oracle in a child process with a time limit and a pair is kept only below MAX_POPS.  What is kept must, over the set
and on BOTH rings, pop each of the four corner cells and enter goals by +x, -x, +y and -y (counted by the model).  Data only: ring,
poses, cells, pop / push / pose counts."""
import json, multiprocessing as mp, os, sys
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import astar_edge_cases as ec


def candidates(key, along_x, along_y, turn, overshoot=0.03):
    """(start cell, goal cell, goal pose or None) -- from every corner: to a goal along each of its two edges, from an edge to the corner
    itself, and round the corner one row / column in; then a goal LESS THAN A CELL outside the grid on each negative side, which the
    reference's truncating cast lands in column 0 / row 0 (grid_utils.hpp:33-38)"""
    W, H = key[1], key[2]
    out = []
    for cx, cy in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)):
        ix, iy = (1 if cx == 0 else -1), (1 if cy == 0 else -1)
        out.append(((cx, cy), (cx + ix * along_x, cy), None))
        out.append(((cx, cy), (cx, cy + iy * along_y), None))
        out.append(((cx + ix * along_x, cy), (cx, cy), None))
        out.append(((cx, cy + iy * along_y), (cx, cy), None))
        out.append(((cx + ix * turn, cy + iy), (cx + ix, cy + iy * turn), None))
        out.append(((cx, cy + iy * turn), (cx + ix * turn, cy), None))
    ox, oy = key[4], key[5]
    out.append(((along_x, 0), (0, 0), (ox - overshoot, oy - overshoot)))
    out.append(((0, along_y), (0, 2), (ox - overshoot, ec.centre(oy, 2))))
    out.append(((along_x, 0), (2, 0), (ec.centre(ox, 2), oy - overshoot)))
    return out


def one(args, q):
    import oracle_lib
    key, sp, gp = args
    orc = oracle_lib.load_oracle()
    r = ec.reference(orc, ec.Case("probe", key, sp, gp, ec.FLAT, None, None, None))
    q.put((r["stats"][0], r["stats"][1], len(r["path"])))


if __name__ == "__main__":
    import oracle_lib
    orc = oracle_lib.load_oracle()
    out = []
    for key, args in ((ec.RING_SMALL, (25, 15, 12)), (ec.RING_LARGE, (300, 200, 40))):
        w = ec.world(key)
        dist = orc.set_distances(w.cells, ec.MPC, ec.helpers.CPM_DEFAULT, w.origin)
        corners, moves, kept = set(), set(), 0
        for sc, gc, gpose in candidates(key, *args):
            sp = (ec.centre(w.origin[0], sc[0]), ec.centre(w.origin[1], sc[1]))
            gp = gpose or (ec.centre(w.origin[0], gc[0]), ec.centre(w.origin[1], gc[1]))
            q = mp.Queue()
            p = mp.Process(target=one, args=((key, sp, gp), q))
            p.start(); p.join(20.0)
            if p.is_alive():
                p.terminate(); p.join()
                print("time limit:", key[1:4], sc, gc, flush=True)
                continue
            pops, pushes, n = q.get()
            if pops > ec.MAX_POPS or n < 2:
                print("dropped:", key[1:4], sc, gc, pops, n, flush=True)
                continue
            m = ec.model(dist, w.origin, sp, gp, ec.FLAT)
            assert (m["pops"], m["pushes"], m["poses"]) == (pops, pushes, n), (sc, gc, m, pops, pushes, n)
            corners |= set(m["corner_pops"]); moves.add(m["last_move"]); kept += 1
            out.append({"ring": list(key[1:4]), "origin": list(key[4:6]), "start": list(sp), "goal": list(gp), "start_cell": list(sc),
                        "goal_cell": list(gc), "pops": pops, "pushes": pushes, "poses": n})
            print(out[-1], sorted(m["corner_pops"]), m["last_move"], flush=True)
        assert kept >= 8 and len(corners) == 4 and len(moves) == 4, (key, kept, corners, moves)
    json.dump(out, open(ec.RING_JSON, "w"), indent=0)
    print(len(out), "cases")
