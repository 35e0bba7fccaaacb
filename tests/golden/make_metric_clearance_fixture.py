"""Writes tests/golden/metric_clearance_gap.txt: what tests/cpp/metric_clearance_test.cpp expects on the diagonal-gap maps, by the
models (tests/edt_model.py, nav_field_model.py).  Run from the repository root: python tests/golden/make_metric_clearance_fixture.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import edt_model as em  # noqa: E402
import nav_field_model as nm  # noqa: E402
import test_edt_model_cpu as cpu  # noqa: E402

ORIGIN, MPC = (np.float32(-1.0), np.float32(-1.0)), np.float32(0.05)
CPM = np.float32(1.0 / np.float64(MPC))


def fnv1a64(data):
    h = 0xCBF29CE484222325
    for b in data:
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def centre(cell):
    return (np.float32(float(ORIGIN[0]) + (cell[0] + 0.5) * float(MPC)), np.float32(float(ORIGIN[1]) + (cell[1] + 0.5) * float(MPC)))


def values():
    out = [("max_cells", cpu.GAP_R)]
    p = cpu.GAP_PARAMS
    sx, sy = centre(cpu.GAP_START)
    for offset in (5, 7):
        cells = cpu.gap_cells(offset)
        code = em.codes(cells, cpu.GAP_R)
        out.append(("codes_fnv_%d" % offset, fnv1a64(code.astype("<u2").tobytes())))
        l1 = nm.l1_distances(cells)
        out.append(("l1_codes_fnv_%d" % offset, fnv1a64(l1.astype("<u2").tobytes())))
        f_l1, f_eu = cpu.gap_fields(offset)
        for tag, dist, f, field in (("l1", l1, nm.dist_table(40, 40), f_l1), ("euclid", code, em.table(cpu.GAP_R, MPC), f_eu)):
            trav, pen = nm.tables(f, p)
            poses, _, cost = nm.descend(field, dist, trav, pen, [cpu.GAP_GOAL], 0, (0, sx, sy, np.float32(0.0)), ORIGIN, MPC, CPM)
            out.append(("%s_cost_%d" % (tag, offset), int(cost)))
            out.append(("%s_len_%d" % (tag, offset), len(poses)))
    out.append(("table_n", cpu.GAP_R * cpu.GAP_R + 2))
    return out


def text():
    return "".join("%s %d\n" % kv for kv in values())


if __name__ == "__main__":
    with open(os.path.join(HERE, "metric_clearance_gap.txt"), "w") as f:
        f.write(text())
