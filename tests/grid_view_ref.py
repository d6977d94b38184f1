"""The ground plan view's contract (include/svo.h, "Ground plan view") restated twice, by two routes that share no code,
both applied to an (na, nb) uint8 `cls` grid, a list of uint32 `views` and an optional (na, nb) uint32 `cost`:

  views_py   cell by cell in Python integers: every target of the square around a view in raster order, rule 3's line by its closed
             formula at every step, the tallies, the cover and the score in Python, the order by sorted();
  views_np   whole arrays in numpy: all targets of a view at once as offset arrays, a loop over the step i that moves every line that
             is still alive by one cell, the cover by np.minimum, the order by np.lexsort.

Neither is the ring-ordered, remainder-stepping walk of the kernels.  Both return a Result: records (a structured array of RECORD, one
per view), order (n_views,) uint32, best (4,) uint32, seen (na, nb) uint32 and the seven counts (n_used, n_ignored, n_in_range,
n_visible, n_gain, n_covered, n_gain_covered).  `variant` of views_np states one deliberate misreading of the contract each;
tests/test_grid_view.py shows that every one of them changes a result.  views_np also counts, into `stats`, the targets in range and
the steps walked towards them (what the measurement reports as work done).  Also here: the seeded random cases and the constructed ones
with the facts they were built for.  Nothing here is tuned on the library's output.
"""
from collections import namedtuple

import numpy as np

Params = namedtuple("Params", "na nb opaque_mask gain_mask max_range gain_weight cost_div")
Result = namedtuple("Result", "records order best seen counts")
Case = namedtuple("Case", "cls views cost prm")
NONE = 0xFFFFFFFF
MAX_SCORE = 0xFFFFFFFE
UNKNOWN, LEVEL, OBSTACLE = 0, 1, 2
RECORD = np.dtype([("cell", "<u4"), ("n_visible", "<u4"), ("n_gain", "<u4"), ("n_opaque", "<u4"), ("cost", "<u4"), ("score", "<u4"),
                   ("reserved", "<u4", (2,))])
VARIANTS = ("tie_towards", "range_lt", "opaque_target_hidden", "open_corners", "either_corner", "no_occlusion", "no_self",
            "order_drop_ignored", "order_largest", "none_zero", "score_wraps")
PY_MAX_RANGE = 62  # views_py leaves out the cases with max_range >= 63, and nothing else


def params(cls, opaque_mask=1 << OBSTACLE, gain_mask=1 << UNKNOWN, max_range=12, gain_weight=16, cost_div=1):
    return Params(cls.shape[0], cls.shape[1], opaque_mask, gain_mask, max_range, gain_weight, cost_div)


def _score(n_gain, cost, has_cost, prm, variant=None):
    if has_cost and cost == NONE:
        if variant != "none_zero":
            return 0
        cost = 0
    g = prm.gain_weight * n_gain
    c = cost // prm.cost_div if has_cost else 0
    if g <= c:
        return (g - c) & NONE if variant == "score_wraps" else 0
    return min(g - c, MAX_SCORE)


def _finish(prm, views, cost, used, tallies, seen, gain, n_in, variant=None):
    """used: per view; tallies: per view (n_visible, n_gain, n_opaque); seen (na, nb) int64; gain (na, nb) bool"""
    nv = len(views)
    rec = np.zeros(nv, RECORD)
    scores = []
    for i in range(nv):
        if not used[i]:
            rec[i] = (NONE, 0, 0, 0, NONE, 0, (0, 0))
            scores.append(0)
            continue
        v = int(views[i])
        c = NONE if cost is None else int(cost.ravel()[v])
        s = _score(tallies[i][1], c, cost is not None, prm, variant)
        rec[i] = (v, tallies[i][0], tallies[i][1], tallies[i][2], c, s, (0, 0))
        scores.append(s)
    ranked = [i for i in range(nv) if used[i] or variant != "order_drop_ignored"]
    ranked.sort(key=lambda i: (-scores[i], -i if variant == "order_largest" else i))
    order = np.full(nv, NONE, np.uint32)
    order[:len(ranked)] = ranked
    first = ranked[0] if ranked else None
    if first is not None and scores[first] > 0:
        best = np.array([rec[first]["cell"], first, scores[first], rec[first]["n_gain"]], np.uint32)
    else:
        best = np.array([NONE, NONE, 0, 0], np.uint32)
    covered = seen != NONE
    counts = (sum(used), nv - sum(used), n_in, sum(t[0] for t in tallies), sum(t[1] for t in tallies), int(covered.sum()),
              int((covered & gain).sum()))
    return Result(rec, order, best, seen.astype(np.uint32), counts)


# ------------------------------------------------------------------------------------------------ route (a): cell by cell
def views_py(cls, views, cost, prm):
    na, nb, R = prm.na, prm.nb, prm.max_range
    assert R <= PY_MAX_RANGE
    n = na * nb
    K = [int(v) for v in np.asarray(cls).ravel()]
    opaque = [k < 32 and (prm.opaque_mask >> k) & 1 == 1 for k in K]
    gain = [k < 32 and (prm.gain_mask >> k) & 1 == 1 for k in K]
    seen = [NONE] * n
    used, tallies, n_in = [], [], 0
    sgn = lambda x: (x > 0) - (x < 0)
    for i, v in enumerate(int(x) for x in views):
        if v >= n or opaque[v]:
            used.append(False)
            tallies.append((0, 0, 0))
            continue
        used.append(True)
        va, vb = divmod(v, nb)
        nvis = ngain = nopq = 0
        for ta in range(max(0, va - R), min(na, va + R + 1)):
            for tb in range(max(0, vb - R), min(nb, vb + R + 1)):
                da, db = ta - va, tb - vb
                if da * da + db * db > R * R:
                    continue
                n_in += 1
                m = max(abs(da), abs(db))
                ok = True
                pa, pb = va, vb
                for s in range(1, m + 1):
                    qa = va + sgn(da) * ((2 * s * abs(da) + m) // (2 * m))
                    qb = vb + sgn(db) * ((2 * s * abs(db) + m) // (2 * m))
                    if qa != pa and qb != pb and opaque[qa * nb + pb] and opaque[pa * nb + qb]:
                        ok = False
                        break
                    if s < m and opaque[qa * nb + qb]:
                        ok = False
                        break
                    pa, pb = qa, qb
                if not ok:
                    continue
                t = ta * nb + tb
                nvis += 1
                ngain += gain[t]
                nopq += opaque[t]
                seen[t] = min(seen[t], i)
        tallies.append((nvis, ngain, nopq))
    return _finish(prm, views, None if cost is None else np.asarray(cost, np.uint32), used, tallies,
                   np.array(seen, np.int64).reshape(na, nb), np.array(gain, bool).reshape(na, nb), n_in)


# ------------------------------------------------------------------------------------------------ route (b): whole arrays
def views_np(cls, views, cost, prm, variant=None, stats=None):
    assert variant is None or variant in VARIANTS, variant
    na, nb, R = prm.na, prm.nb, prm.max_range
    n = na * nb
    cls = np.asarray(cls, np.uint8).reshape(na, nb)
    k = np.minimum(cls, 31).astype(np.uint32)
    known = cls < 32
    opaque = known & (((np.uint32(prm.opaque_mask) >> k) & 1) == 1)
    gain = known & (((np.uint32(prm.gain_mask) >> k) & 1) == 1)
    seen = np.full((na, nb), NONE, np.int64)
    off = np.arange(-R, R + 1, dtype=np.int64)
    DA, DB = (x.ravel() for x in np.meshgrid(off, off, indexing="ij"))
    D2 = DA * DA + DB * DB
    near = D2 < R * R if variant == "range_lt" else D2 <= R * R
    used, tallies, n_in, steps = [], [], 0, 0
    for i, v in enumerate(int(x) for x in views):
        if v >= n or opaque.ravel()[v]:
            used.append(False)
            tallies.append((0, 0, 0))
            continue
        used.append(True)
        va, vb = divmod(v, nb)
        inside = near & (va + DA >= 0) & (va + DA < na) & (vb + DB >= 0) & (vb + DB < nb)
        if variant == "no_self":
            inside &= D2 > 0
        da, db = DA[inside], DB[inside]
        n_in += len(da)
        ada, adb = np.abs(da), np.abs(db)
        sa, sb = np.sign(da), np.sign(db)
        m = np.maximum(ada, adb)
        m1 = np.maximum(m, 1)
        alive = np.ones(len(da), bool)
        pa, pb = np.full(len(da), va), np.full(len(da), vb)
        for s in range(1, int(m.max()) + 1 if len(m) else 1):
            go = alive & (m >= s)
            steps += int(go.sum())
            if variant == "tie_towards":
                qa, qb = va + sa * ((2 * s * ada + m1 - 1) // (2 * m1)), vb + sb * ((2 * s * adb + m1 - 1) // (2 * m1))
            else:
                qa, qb = va + sa * ((2 * s * ada + m1) // (2 * m1)), vb + sb * ((2 * s * adb + m1) // (2 * m1))
            qa, qb = np.where(go, qa, pa), np.where(go, qb, pb)  # a line that has ended, or was stopped, stays where it is
            diag = go & (qa != pa) & (qb != pb)
            side1, side2 = opaque[qa, pb], opaque[pa, qb]
            if variant == "open_corners":
                corner = np.zeros(len(da), bool)
            elif variant == "either_corner":
                corner = diag & (side1 | side2)
            else:
                corner = diag & side1 & side2
            inner = go & (m > s) & opaque[qa, qb]
            if variant == "no_occlusion":
                corner, inner = corner & False, inner & False
            alive &= ~(corner | inner)
            pa, pb = qa, qb
        ta, tb = va + da[alive], vb + db[alive]
        if variant == "opaque_target_hidden":
            keep = ~opaque[ta, tb]
            ta, tb = ta[keep], tb[keep]
        tallies.append((len(ta), int(gain[ta, tb].sum()), int(opaque[ta, tb].sum())))
        seen[ta, tb] = np.minimum(seen[ta, tb], i)
    if stats is not None:
        stats["targets"] = stats.get("targets", 0) + n_in
        stats["steps"] = stats.get("steps", 0) + steps
    return _finish(prm, views, None if cost is None else np.asarray(cost, np.uint32), used, tallies, seen, gain, n_in, variant)


def same(x, y):
    return x.records.tobytes() == y.records.tobytes() and np.array_equal(x.order, y.order) and np.array_equal(x.best, y.best) and \
        np.array_equal(x.seen, y.seen) and tuple(x.counts) == tuple(y.counts)


# ------------------------------------------------------------------------------------------------ cases
SHARED = dict(opaque_mask=(1 << OBSTACLE) | (1 << UNKNOWN), gain_mask=1 << UNKNOWN)  # the conservative gain


def random_grid(na, nb, p_unknown, p_obstacle, rng):
    u = rng.random((na, nb))
    return np.where(u < p_unknown, UNKNOWN, np.where(u < p_unknown + p_obstacle, OBSTACLE, LEVEL)).astype(np.uint8)


def random_case(na, nb, p_unknown, p_obstacle, n_views, max_range, seed=None, with_cost=True, kinds=True, **prm):
    """cls drawn per cell; views drawn among the LEVEL cells (all cells where there is none); with `kinds` and eight views or more:
    every fourth a duplicate of an earlier one, the last eighth 0xFFFFFFFF padding, one index just outside the grid, one 2^31 and one on
    an OBSTACLE cell where there is one.  cost seeded below 2048 (gains of 16 a cell lie on both sides), a quarter of it NONE."""
    rng = np.random.default_rng(1000 * na + nb + 7 * max_range if seed is None else seed)
    cls = random_grid(na, nb, p_unknown, p_obstacle, rng)
    n = na * nb
    level = np.flatnonzero(cls.ravel() == LEVEL)
    pool = level if len(level) else np.arange(n)
    views = pool[rng.integers(0, len(pool), n_views)].astype(np.uint32)
    if kinds and n_views >= 8:
        views[3::4] = views[1:n_views - 2:4][:len(views[3::4])]
        views[n_views - n_views // 8:] = NONE
        views[1], views[5] = n, 1 << 31
        walls = np.flatnonzero(cls.ravel() == OBSTACLE)
        if len(walls):
            views[2] = walls[len(walls) // 2]
    cost = rng.integers(0, 2048, (na, nb)).astype(np.uint32)
    cost[rng.random((na, nb)) < 0.25] = NONE
    return Case(cls, views, cost if with_cost else None, params(cls, max_range=max_range, **prm))


def corner_case(na, nb, max_range, seed=3):
    """views in the four corners of the grid (made LEVEL), then the middle"""
    rng = np.random.default_rng(seed + 1000 * na + nb)
    cls = random_grid(na, nb, 0.3, 0.08, rng)
    n = na * nb
    views = np.array([0, nb - 1, n - nb, n - 1, (na // 2) * nb + nb // 2], np.uint32)
    cls.ravel()[views] = LEVEL
    return Case(cls, views, None, params(cls, max_range=max_range))


def _room(size, wall):
    """UNKNOWN outside, LEVEL inside, OBSTACLE where wall(da, db) holds, seen from the centre"""
    c = size // 2
    cls = np.full((size, size), UNKNOWN, np.uint8)
    for a in range(size):
        for b in range(size):
            w = wall(a - c, b - c)
            cls[a, b] = OBSTACLE if w == 0 else (LEVEL if w < 0 else UNKNOWN)
    return cls, np.array([c * size + c], np.uint32)


def constructed():
    """name -> (case, facts): facts["records"] {view: {field: value}}, facts["visible"] / facts["hidden"]: cells (ia, ib) that view 0
    sees / does not see, facts["counts"] the seven counts"""
    out = {}
    L, U, O = LEVEL, UNKNOWN, OBSTACLE
    # a room closed by a one-cell square wall at Chebyshev distance 3: the 5 x 5 inside and the wall's 20 cells that are no corner (the
    # last step to a corner passes between two wall cells), nothing outside; only the grid's four corners are out of range 8
    cls, views = _room(13, lambda da, db: max(abs(da), abs(db)) - 3)
    out["closed_room"] = (Case(cls, views, None, params(cls, max_range=8)),
                          {"records": {0: {"n_visible": 45, "n_gain": 0, "n_opaque": 20, "cost": NONE, "score": 0}},
                           "counts": (1, 0, 13 * 13 - 4, 45, 0, 45, 0), "hidden": [(6, 2), (2, 2), (1, 6), (12, 12), (3, 3), (9, 3)],
                           "visible": [(3, 4), (6, 3), (9, 8), (4, 4)]})
    # a wall of the cells at Manhattan distance 3: its cells touch only diagonally, and only the corner rule closes it: 1 + 4 + 8 + 12
    cls, views = _room(13, lambda da, db: abs(da) + abs(db) - 3)
    out["diamond_room"] = (Case(cls, views, None, params(cls, max_range=8)),
                           {"records": {0: {"n_visible": 25, "n_gain": 0, "n_opaque": 12}}, "hidden": [(4, 4), (6, 2), (8, 8), (3, 7)],
                            "visible": [(5, 5), (6, 3), (4, 5)]})
    # one pillar three cells along the row and its shadow behind it
    cls = np.full((11, 16), L, np.uint8)
    cls[5, 8] = O
    out["pillar"] = (Case(cls, np.array([5 * 16 + 5], np.uint32), None, params(cls, max_range=10)),
                     {"records": {0: {"n_opaque": 1, "n_gain": 0}}, "visible": [(5, 8), (5, 7), (4, 9), (6, 9), (5, 0)],
                      "hidden": [(5, 9), (5, 10), (5, 15)]})
    # a wall with a one-cell door, UNKNOWN behind it: the view looks through the door along its row only
    cls = np.full((11, 12), L, np.uint8)
    cls[:, 7:] = U
    cls[:, 6] = O
    cls[5, 6] = L
    out["door"] = (Case(cls, np.array([5 * 12 + 3], np.uint32), None, params(cls, max_range=10)),
                   {"visible": [(5, 6), (5, 7), (5, 11), (0, 6), (10, 6)], "hidden": [(0, 9), (10, 7), (2, 11)]})
    # the target (2, 1) from (0, 0): n = 2, L_1 = (1, floor((2 + 2) / 4)) = (1, 1), the tie rounded away from V
    cls = np.array([[L, L, L], [L, O, L], [L, U, L]], np.uint8)
    out["tie_blocked"] = (Case(cls, np.array([0], np.uint32), None, params(cls, max_range=3)), {"hidden": [(2, 1), (1, 2), (2, 2)], "visible": [(1, 1), (2, 0)]})
    cls = np.array([[L, L, L], [O, L, L], [L, U, L]], np.uint8)
    out["tie_open"] = (Case(cls, np.array([0], np.uint32), None, params(cls, max_range=3)),
                       {"visible": [(2, 1), (1, 0)], "hidden": [(2, 0)], "records": {0: {"n_gain": 1, "score": 16}}})
    # every kind of entry, a cost on both sides of the gain, a tie in the score: U row seen by all three used views
    cls = np.array([[L, L, L, L], [U, U, U, U], [O, L, L, L]], np.uint8)
    cost = np.array([[0, 16 * 4 + 5, NONE, 7], [0, 0, 0, 0], [0, 0, 0, 0]], np.uint32)
    views = np.array([3, NONE, 8, 1, 12, 0, 2, 0], np.uint32)
    out["kinds_and_scores"] = (Case(cls, views, cost, params(cls, max_range=8)),
                               {"records": {0: {"cell": 3, "cost": 7, "n_gain": 4, "score": 57}, 1: {"cell": NONE, "score": 0, "cost": NONE},
                                            2: {"cell": NONE}, 3: {"cell": 1, "n_gain": 4, "score": 0}, 4: {"cell": NONE},
                                            5: {"cell": 0, "score": 64}, 6: {"cell": 2, "cost": NONE, "score": 0}, 7: {"score": 64}},
                                "order": [5, 7, 0, 1, 2, 3, 4, 6], "best": (0, 5, 64, 4)})
    return out


def misreading_case():
    """63 x 65, seed 7, 12 views at range 12 over a tenth of obstacles and a third of unknown ground, with every kind of entry, a
    duplicate (a tie in the score), an unreachable view and one whose cost exceeds its gain."""
    rng = np.random.default_rng(7)
    na, nb = 63, 65
    cls = random_grid(na, nb, 0.3, 0.15, rng)
    level = np.flatnonzero(cls.ravel() == LEVEL)
    views = level[rng.integers(0, len(level), 12)].astype(np.uint32)
    views[6] = views[0]
    views[9], views[10] = NONE, na * nb
    views[11] = np.flatnonzero(cls.ravel() == OBSTACLE)[5]
    cost = rng.integers(0, 512, (na, nb)).astype(np.uint32)
    cost.ravel()[views[2]] = NONE
    cost.ravel()[views[3]] = 1 << 20
    return Case(cls, views, cost, params(cls, max_range=12))
