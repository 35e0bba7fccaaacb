"""Hand-built clouds for bl_pf_clusters: (x, y, theta, units) arrays with the parameters they are meant for.  Positions are
placed in bins of 0.25 m (a power of two: bin edges are exact floats), headings in the middle of a heading bin."""
import math

import numpy as np

BIN = 0.25
T36 = 36


def _mid(i, bin_xy=BIN):
    return (np.asarray(i, np.float64) + 0.5) * bin_xy


def _heading(it, T):
    return (np.asarray(it, np.float64) + 0.5) * (2.0 * math.pi / T)


def _case(x, y, th, units, bin_xy=BIN, T=T36, K=8):
    x, y, th = (np.asarray(a, np.float64).astype(np.float32) for a in (x, y, th))
    n = len(x)
    assert len(y) == n and len(th) == n and len(units) == n
    return {"x": x, "y": y, "th": th, "units": np.asarray(units, np.uint64).astype(np.uint32), "bin_xy": bin_xy, "T": T, "K": K}


def in_bins(cells, units=None, bin_xy=BIN, T=T36, K=8, jitter=None):
    """One particle in the middle of each (ix, iy, it) given."""
    c = np.asarray(cells, np.int64).reshape(-1, 3)
    u = np.ones(len(c), np.uint32) if units is None else units
    x, y = _mid(c[:, 0], bin_xy), _mid(c[:, 1], bin_xy)
    if jitter is not None:
        x, y = x + jitter[0], y + jitter[1]
    return _case(x, y, _heading(c[:, 2], T), u, bin_xy, T, K)


def one_bin(n):
    """Every particle in one bin (maximal contention), spread inside it, with unequal units."""
    i = np.arange(n)
    return _case(0.26 + (i % 97) * 0.002, -0.49 + (i % 89) * 0.002, 0.20 + (i % 7) * 0.01, 1 + (i * 2654435761) % 1000, K=4)


def isolated(n):
    """Every particle in a bin of its own, none adjacent: C = n, many equal U -- the order falls to the anchors."""
    i = np.arange(n)
    w = 64
    return in_bins(np.stack([2 * (i % w) - 40, 2 * (i // w) - 30, (5 * i) % T36], 1), units=1 + (i % 3), K=64)


def snake():
    """A diagonal of 2000 bins, the heading stepping along: one cluster."""
    i = np.arange(2000)
    return in_bins(np.stack([i - 1000, i - 1000, i % T36], 1))


def two_snakes():
    """Two rows of 1500 bins with exactly one empty row between them, walked in opposite directions: two clusters."""
    i = np.arange(1500)
    a = np.stack([i, 0 * i, i % T36], 1)
    b = np.stack([i[::-1], 0 * i + 2, i % T36], 1)
    return in_bins(np.concatenate([a, b]), units=np.concatenate([np.full(1500, 2), np.full(1500, 3)]))


def ring():
    """The border of a square of 60 x 60 bins and, at one cell apart from it, every heading bin: two rings, two clusters."""
    s = 60
    border = [(i, 0, 0) for i in range(s)] + [(s - 1, j, 0) for j in range(1, s)] + [(i, s - 1, 0) for i in range(s - 1)] + \
             [(0, j, 0) for j in range(1, s - 1)]
    headings = [(30, 30, t) for t in range(T36)]
    return in_bins(border + headings)


def heading_wrap(other):
    """it = 0 and it = other at one cell (T = 36)."""
    return in_bins([(3, 3, 0), (3, 3, other)])


def small_T(T):
    """T = 1, 2, 3: headings all round the circle at one cell and at a diagonal neighbour, and a cell apart from both."""
    th = np.array([-3.0, -2.0, -1.0, -0.1, 0.0, 0.1, 1.0, 2.0, 3.0, 0.5, 2.5, -2.5, 1.2])
    x = _mid([0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 5])
    y = _mid([0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 5])
    return _case(x, y, th, np.arange(1, len(th) + 1), T=T)


def heading_values():
    """+-pi to the float, -0.0, 99.9, 100.0 (no heading terms from there on), a NaN, an infinity."""
    pi = np.float32(math.pi)
    th = np.array([pi, -pi, -0.0, 0.0, 99.9, 100.0, -100.0, np.nextafter(np.float32(100.0), np.float32(0.0)), 1e6, np.nan, np.inf, -np.inf],
                  np.float32)
    n = len(th)
    return _case(np.full(n, 0.1), np.full(n, 0.1), th.astype(np.float64), np.arange(1, n + 1) * 1000)


def position_edges():
    """x just below and at a bin boundary on both sides of 0 (floor, not truncation), beyond the clamp, NaN."""
    f = np.float32
    xs = [np.nextafter(f(0.25), f(0)), f(0.25), np.nextafter(f(-0.25), f(-1)), f(-0.25), np.nextafter(f(-0.25), f(0)), f(0.0), f(-0.0),
          np.nextafter(f(0), f(-1)), np.nextafter(f(0), f(1)), f(1e9), f(-1e9), f(np.inf), f(-np.inf), f(np.nan), f(262143.9), f(-262144.0)]
    xs = np.array(xs, np.float32)
    n = len(xs)
    c = _case(xs.astype(np.float64), np.full(n, 0.1), np.full(n, 0.2), np.arange(1, n + 1))
    c["y"][5] = np.float32(np.nan)
    return c


def bridges():
    """Two weighted groups joined only by zero-unit particles (one cluster, the bridges add no weight), and a cluster of zero-unit
    particles alone (it sorts last and has no pose)."""
    cells = [(0, 0, 0), (1, 0, 0), (2, 0, 1), (3, 0, 1), (4, 1, 2), (5, 1, 2), (6, 1, 2), (7, 1, 3),
             (20, 20, 9), (21, 20, 9), (-9, -9, 0)]
    units = [5, 7, 9, 0, 0, 0, 11, 13, 0, 0, 4]
    return in_bins(cells, units=units)


def big_units():
    """4097 particles of 2^32 - 1 units near x = y = 500 m, bins of 0.05 m: the second moments need more than 64 bits."""
    i = np.arange(4097)
    return _case(500.0 + (i % 64) * 0.003, 500.0 + (i // 64) * 0.003, 0.1 * (i % 5), np.full(4097, 2 ** 32 - 1, np.uint64), bin_xy=0.05)


def three_clusters(K):
    return in_bins([(0, 0, 0), (1, 0, 0), (10, 0, 0), (10, 1, 1), (10, 2, 2), (-10, 5, 7)], units=[4, 4, 1, 2, 3, 9], K=K)


def hundred_clusters():
    """C = 100 with K = 8, units that order them against their anchors."""
    i = np.arange(100)
    return in_bins(np.stack([3 * (i % 10), 3 * (i // 10), 0 * i], 1), units=1 + (i * 37) % 101, K=8)


def bimodal():
    """70 % of the units around A = (1.0, 2.0, 0.5), 30 % around B, 4 m further along x."""
    rng = np.random.default_rng(12)
    na, nb = 1400, 600
    x = np.concatenate([1.0 + 0.03 * rng.standard_normal(na), 5.0 + 0.03 * rng.standard_normal(nb)])
    y = np.concatenate([2.0 + 0.03 * rng.standard_normal(na), 2.0 + 0.03 * rng.standard_normal(nb)])
    th = np.concatenate([0.5 + 0.05 * rng.standard_normal(na), -1.0 + 0.05 * rng.standard_normal(nb)])
    return _case(x, y, th, np.full(na + nb, 5), bin_xy=0.5)


LAUNCH_SIZES = (2, 63, 64, 65, 1023, 1024, 1025, 4097)


def all_cases():
    """name -> case, every hand-built cloud (the launch-edge sizes included)."""
    c = {}
    for n in LAUNCH_SIZES:
        c["one_bin_%d" % n] = one_bin(n)
        c["isolated_%d" % n] = isolated(n)
    c.update(snake=snake(), two_snakes=two_snakes(), ring=ring(), wrap_35=heading_wrap(35), wrap_34=heading_wrap(34),
             T1=small_T(1), T2=small_T(2), T3=small_T(3), heading_values=heading_values(), position_edges=position_edges(),
             bridges=bridges(), big_units=big_units(), K1=three_clusters(1), K64=three_clusters(64), C100=hundred_clusters(),
             bimodal=bimodal())
    return c
