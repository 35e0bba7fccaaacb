"""The model of the Euclidean distance grid (include/botlab_hip.h, "Euclidean distance grid"), restated in Python: the definition the
kernels of botlab_amd/csrc/bl_edt.hip are checked against, code for code.  Integers throughout; the float table is formed in double
with numpy's correctly rounded sqrt.

  row_pass     g(x, y): the distance along the row to the nearest source of that row, capped at R + 1
  codes        THE MODEL: the row pass, then the minimum over |dy| <= R of g(x, y + dy)^2 + dy^2, then the cap
  brute_force  a second, independent form: the minimum over all sources, cell by cell
  table        f[k] = (float)(sqrt((double)k) * (double)meters_per_cell), k = 0 .. R^2 + 1
  floats       the float view: f[code], -1 where the map has no source
"""
import numpy as np

NONE16 = 0xFFFF
MAX_CELLS = 254


def far(R):
    return R * R + 1


def row_pass(cells, R):
    """int64 (h, w): min(distance to the nearest source in the row, R + 1)."""
    h, w = cells.shape
    cap = R + 1
    g = np.where(cells >= 0, 0, cap).astype(np.int64)
    for x in range(1, w):
        g[:, x] = np.minimum(g[:, x], g[:, x - 1] + 1)
    for x in range(w - 2, -1, -1):
        g[:, x] = np.minimum(g[:, x], g[:, x + 1] + 1)
    return np.minimum(g, cap)


def codes(cells, R):
    """THE MODEL.  uint16 (h, w)."""
    assert 1 <= R <= 255                                          # (the library stops at MAX_CELLS: its row pass keeps R + 1 in a byte)
    cells = np.asarray(cells)
    h, w = cells.shape
    if not (cells >= 0).any():
        return np.full((h, w), NONE16, np.uint16)
    g = row_pass(cells, R)
    cap = R + 1
    pad = np.full((h + 2 * R, w), cap, np.int64)                  # rows outside the grid hold no source
    pad[R:R + h] = g
    best = g * g
    for dy in range(1, R + 1):
        up, down = pad[R - dy:R - dy + h], pad[R + dy:R + dy + h]
        m = np.minimum(up, down)
        best = np.minimum(best, m * m + dy * dy)
    return np.where(best <= R * R, best, far(R)).astype(np.uint16)


def brute_force(cells, R):
    """The same codes from the definition: every cell against every source."""
    cells = np.asarray(cells)
    h, w = cells.shape
    ys, xs = np.nonzero(cells >= 0)
    if len(xs) == 0:
        return np.full((h, w), NONE16, np.uint16)
    out = np.zeros((h, w), np.uint16)
    xs, ys = xs.astype(np.int64), ys.astype(np.int64)
    for y in range(h):
        for x in range(w):
            d2 = int(((xs - x) ** 2 + (ys - y) ** 2).min())
            out[y, x] = d2 if d2 <= R * R else far(R)
    return out


def table(R, mpc):
    k = np.arange(R * R + 2, dtype=np.float64)
    return (np.sqrt(k) * np.float64(np.float32(mpc))).astype(np.float32)


def floats(code, f):
    return np.where(code == NONE16, np.float32(-1.0), f[np.minimum(code, len(f) - 1)]).astype(np.float32)
