"""The model of loop closure by place recognition (bl_loopclose_find_places, include/botlab_hip.h, "loop closure by place recognition";
DESIGN.md 4.34).  TEST INFRASTRUCTURE, no GPU.

The definition restated in numpy: the descriptors (float32 products, truncation, bits), the best pair of every query over all older
scans and all 64 shifts in integers, the centre of the match in float32 with every operation rounded by itself.  The candidate list is
composed from loop_closure_model's submap, gate, edge and records and scan_match_prior_model.match, which are used as they are.  The
device must reproduce every field bit for bit.

The all-pairs part has no Python loop over (q, j, s): the descriptors are spread into 2048 bit planes of float32 and the overlaps of all
queries with all partners at one shift are one matrix product, whose sums of at most 2048 ones are exact in float32."""
import numpy as np

import loop_closure_model as lcm

smp = lcm.smp
F32 = np.float32
SECTORS, BINS = 64, 32
K = F32(10.185916)                      # the float nearest 32 / pi
STEP = F32(0.09817477)                  # the float nearest 2 pi / 64
MAX_THETA = F32(1024.0)
MIN_RANGE = smp.sm.MIN_RANGE

PLACE_DTYPE = np.dtype([(n, "<i4") for n in ("q", "j", "shift", "key", "overlap", "bits_q", "bits_j", "partner")])
PARAMS_LAYOUT = (("bins_per_meter", 0), ("max_range", 4), ("dilate", 8), ("min_key", 12), ("min_bits", 16), (None, 20))
PLACE_LAYOUT = tuple((n, 4 * i) for i, n in enumerate(PLACE_DTYPE.names)) + ((None, 32),)
PLACE_DEFAULTS = dict(bins_per_meter=4.0, place_max_range=8.0, dilate=1, min_key=16384, min_bits=8)


def check_place(p):
    """True iff bl_loopclose_find_places accepts the place parameters (a dict with PLACE_DEFAULTS' keys)."""
    b, r = F32(p["bins_per_meter"]), F32(p["place_max_range"])
    return bool(b > 0 and b <= 1000 and r > MIN_RANGE and r <= 1000 and p["dilate"] in (0, 1) and 0 <= p["min_key"] <= 65536 and
                0 <= p["min_bits"] <= SECTORS * BINS)


def check_params(p):
    """find's limits without the radius"""
    return lcm.check_params(dict(p, radius=1.0))


# ---------------------------------------------------------------- descriptors
def descriptor(ranges, thetas, bins_per_meter, max_range):
    """uint32 [64] of one scan"""
    r, t = np.asarray(ranges, F32), np.asarray(thetas, F32)
    with np.errstate(invalid="ignore"):
        ok = (r > MIN_RANGE) & (r < F32(max_range)) & (np.abs(t) <= MAX_THETA)       # NaN fails every compare
    r, t = r[ok], t[ok]
    a = np.floor(t * K).astype(np.int64) & (SECTORS - 1)                             # one float32 multiply
    b = np.minimum((r * F32(bins_per_meter)).astype(np.int64), BINS - 1)             # one float32 multiply, truncated
    d = np.zeros(SECTORS, np.uint32)
    np.bitwise_or.at(d, a, (np.uint32(1) << b.astype(np.uint32)).astype(np.uint32))
    return d


def popcount(words):
    """set bits over the last axis"""
    w = np.ascontiguousarray(words, np.uint32)
    return np.unpackbits(w.view(np.uint8), axis=-1).sum(axis=-1).astype(np.int32)


def descriptors(scans, bins_per_meter, max_range):
    """(words uint32 [n][64], bits int32 [n])"""
    d = np.stack([descriptor(s.ranges, s.thetas, bins_per_meter, max_range) for s in scans]) if len(scans) else np.zeros((0, SECTORS), np.uint32)
    return d, popcount(d)


def dilated(d, dilate):
    d = np.asarray(d, np.uint32)
    return d if not dilate else (d | (d << np.uint32(1)) | (d >> np.uint32(1))).astype(np.uint32)


def planes(d):
    """float32 [n][64][32]: bit b of word a"""
    d = np.asarray(d, np.uint32)
    return ((d[..., None] >> np.arange(BINS, dtype=np.uint32)) & np.uint32(1)).astype(F32)


def overlaps(dq, dj):
    """int64 [64]: ov(s) of one pair, word by word -- the definition as it is written, for the tests of best()"""
    dq, dj = np.asarray(dq, np.uint32), np.asarray(dj, np.uint32)
    return np.array([int(popcount(np.roll(dq, -s) & dj)) for s in range(SECTORS)], np.int64)


def key_of(ov, bits_dq, bits_j):
    den = int(bits_dq) + int(bits_j) - int(ov)
    return 0 if den == 0 else (int(ov) * 65536) // den


# ---------------------------------------------------------------- best pairs
def best(d, bits, stride, min_gap, dilate, min_key, min_bits):
    """PLACE_DTYPE [queries]"""
    n = len(d)
    qs = np.arange(0, n, stride)
    out = np.zeros(len(qs), PLACE_DTYPE)
    out["q"], out["bits_q"], out["j"], out["partner"] = qs, bits[qs] if n else 0, -1, -1
    if n == 0:
        return out
    last = qs - min_gap - 1
    nj = max(int(last.max()) + 1, 0)                                               # partners that any query may take
    eligible = (np.arange(nj)[None, :] <= last[:, None]) & (bits[None, :nj] >= min_bits) & (bits[qs] >= min_bits)[:, None]
    live = np.flatnonzero(eligible.any(axis=1))                                    # queries with an eligible partner
    if len(live) == 0:
        return out
    eligible, bits_j = eligible[live], bits[:nj].astype(np.int64)
    dq = dilated(d[qs[live]], dilate)
    bits_dq = popcount(dq).astype(np.int64)
    pj = planes(d[:nj]).reshape(nj, SECTORS * BINS)
    pq = planes(dq)                                                                # [live][64][32]
    bkey = np.full(len(live), -1, np.int64)
    bj, bs, bov = np.zeros(len(live), np.int64), np.zeros(len(live), np.int64), np.zeros(len(live), np.int64)
    rows = np.arange(len(live))
    for s in range(SECTORS):
        ov = (np.roll(pq, -s, axis=1).reshape(len(live), -1) @ pj.T).astype(np.int64)    # word a of the partner meets word a + s
        den = bits_dq[:, None] + bits_j[None, :] - ov
        key = np.where(den == 0, 0, (ov * 65536) // np.maximum(den, 1))
        key = np.where(eligible, key, -1)
        j = key.argmax(axis=1)                                                     # the lowest j of the greatest key
        k = key[rows, j]
        better = (k > bkey) | ((k == bkey) & (j < bj))                             # equal (key, j): the lower s stays
        bkey[better], bj[better], bs[better], bov[better] = k[better], j[better], s, ov[rows, j][better]
    assert (bkey >= 0).all()
    out["j"][live], out["shift"][live], out["key"][live], out["overlap"][live] = bj, bs, bkey, bov
    out["bits_j"][live] = bits[bj]
    out["partner"][live] = np.where(bkey >= min_key, bj, -1)
    return out


def centre(pose_j, shift):
    """(x_j, y_j, theta_j + (float)ss * STEP) in float32, the product and the sum rounded one by one; no wrap"""
    ss = shift if shift < 32 else shift - 64
    return F32(pose_j[0]), F32(pose_j[1]), F32(F32(pose_j[2]) + F32(F32(ss) * STEP))


# ---------------------------------------------------------------- the whole definition
def find(orc, scans, poses, mpc, cpm, with_candidates=True, **kw):
    """scans, poses as loop_closure_model.find takes them.  Returns (words, bits, places, candidates): the candidates are
    loop_closure_model.find's dicts (no d2; `centre` and `shift` added) in ascending q, ready for loop_closure_model.records."""
    place = {k: kw.pop(k, v) for k, v in PLACE_DEFAULTS.items()}
    kw.pop("radius", None)
    p = dict(lcm.DEFAULTS, **kw)
    assert check_params(p) and check_place(place)
    d, bits = descriptors(scans, place["bins_per_meter"], place["place_max_range"])
    places = best(d, bits, p["stride"], p["min_gap"], place["dilate"], place["min_key"], place["min_bits"])
    out = []
    if len(scans) < 2 or not with_candidates:
        return d, bits, places, out
    for pl in places[places["partner"] >= 0]:
        q, j = int(pl["q"]), int(pl["j"])
        cells, origin, first, count = lcm.submap(orc, scans, poses, j, p["w"], p["submap_cells"], mpc, cpm, p["maxLaserDistance"], p["hitOdds"],
                                                 p["missOdds"])
        ctr = centre(poses[j], int(pl["shift"]))
        c = dict(q=q, j=j, first=first, count=count, origin=origin, cells=cells, ref=None, z=None, info=None, flags=lcm.TOO_MANY_RAYS,
                 centre=ctr, shift=int(pl["shift"]))
        c["valid"] = len(smp.sm.valid_rays(scans[q].ranges, scans[q].thetas, p["max_range"])[0])
        if c["valid"] <= lcm.MAX_RAYS:
            ref = smp.match(cells, origin, mpc, cpm, scans[q].ranges, scans[q].thetas, ctr, p["nx"], p["ny"], p["ntheta"], p["dtheta"],
                            p["max_range"], prior=p["prior"], half_life=p["half_life"], min_score=p["min_score"], utime=int(poses[q][3]))
            c["ref"] = ref
            c["flags"] = lcm.gate(ref, p["nx"], p["ny"], p["ntheta"])
            if c["flags"] == 0:
                c["z"], c["info"] = lcm.edge(ref, ctr, poses[j], mpc, p["dtheta"])
        out.append(c)
    return d, bits, places, out
