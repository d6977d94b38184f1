"""The ground plan frontiers' contract (include/svo.h, "Ground plan frontiers") restated twice, by two routes that share no
code, both applied to an (na, nb) uint8 `cls` grid, an optional (na, nb) uint8 `blocked` and an optional (na, nb) uint32 `cost`:

  frontiers_py   cell by cell in Python integers: the frontier test by a loop over the four edge neighbours, the components by a flood
                 fill with an explicit stack in raster order of the seeds (so a component's seed is its first_cell and the kept ones
                 come out in rank order), the statistics accumulated in Python;
  frontiers_np   whole arrays in numpy: the frontier mask from four shifted arrays, the labels by repeated minimum over eight shifted
                 arrays (and a jump through the label) until nothing changes, the statistics by np.unique / np.add.at / np.minimum.at.

Neither is the tiled union-find of the kernels.  Both return a Result: frontiers (a structured array of RECORD with the n_written
records), goal_cells (max_frontiers,) uint32 padded with NONE, label (na, nb) uint32 and the seven counts (n_free, n_unknown,
n_frontier_cells, n_frontiers, n_kept, n_written, n_kept_cells).  `variant` of frontiers_np states one deliberate misreading of the
contract each; tests/test_grid_frontier.py shows that every one of them changes a result.  Also here: the seeded random cases and the
constructed ones with the facts they were built for.  Nothing here is tuned on the library's output.
"""
from collections import namedtuple

import numpy as np

Params = namedtuple("Params", "na nb free_mask unknown_mask min_size max_frontiers")
Result = namedtuple("Result", "frontiers goal_cells label counts")
Case = namedtuple("Case", "cls blocked cost prm")
NONE = 0xFFFFFFFF
UNKNOWN, LEVEL, OBSTACLE = 0, 1, 2
RECORD = np.dtype([("first_cell", "<u4"), ("size", "<u4"), ("rep_cell", "<u4"), ("best_cell", "<u4"), ("best_cost", "<u4"),
                   ("min_a", "<u2"), ("max_a", "<u2"), ("min_b", "<u2"), ("max_b", "<u2"), ("reserved", "<u4"),
                   ("sum_a", "<u8"), ("sum_b", "<u8")])
VARIANTS = ("four", "eight_unknown", "no_blocked", "outside_unknown", "gt_min", "rank_size", "round_centroid", "rep_largest",
            "best_largest", "none_smallest")
SIZES = [(1, 1), (1, 257), (257, 1), (2, 2)] + [(s, s) for s in (15, 16, 17, 31, 32, 33, 63, 64, 65)] + \
        [(33, 15), (65, 31), (63, 65), (130, 300)]
DENSITIES = ((0.05, 0.05), (0.3, 0.1), (0.6, 0.2))  # (p_unknown, p_obstacle)


def params(cls, free_mask=1 << LEVEL, unknown_mask=1 << UNKNOWN, min_size=3, max_frontiers=1024):
    return Params(cls.shape[0], cls.shape[1], free_mask, unknown_mask, min_size, max_frontiers)


def _result(prm, kept, label, tallies):
    """kept: the kept frontiers' records as tuples in rank order, all of them"""
    n_written = min(len(kept), prm.max_frontiers)
    rec = np.zeros(n_written, RECORD)
    for i in range(n_written):
        rec[i] = kept[i]
    goal = np.full(prm.max_frontiers, NONE, np.uint32)
    goal[:n_written] = rec["rep_cell"]
    n_free, n_unknown, n_cells, n_frontiers = tallies
    counts = (n_free, n_unknown, n_cells, n_frontiers, len(kept), n_written, sum(k[1] for k in kept))
    return Result(rec, goal, label, counts)


# ------------------------------------------------------------------------------------------------ route (a): flood fill
def frontiers_py(cls, blocked, cost, prm):
    na, nb = prm.na, prm.nb
    n = na * nb
    K = [int(v) for v in np.asarray(cls).ravel()]
    B = None if blocked is None else [int(v) for v in np.asarray(blocked).ravel()]
    W = None if cost is None else [int(v) for v in np.asarray(cost).ravel()]
    free = [k < 32 and (prm.free_mask >> k) & 1 == 1 and (B is None or B[v] == 0) for v, k in enumerate(K)]
    unknown = [k < 32 and (prm.unknown_mask >> k) & 1 == 1 for k in K]
    front = [False] * n
    for v in range(n):
        if not free[v]:
            continue
        ia, ib = divmod(v, nb)
        for da, db in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            ja, jb = ia + da, ib + db
            if 0 <= ja < na and 0 <= jb < nb and unknown[ja * nb + jb]:
                front[v] = True
                break
    label = [NONE] * n
    seen = [False] * n
    kept = []
    n_frontiers = 0
    for seed in range(n):  # raster order: the seed of a component is its smallest cell
        if not front[seed] or seen[seed]:
            continue
        n_frontiers += 1
        members, stack = [], [seed]
        seen[seed] = True
        while stack:
            v = stack.pop()
            members.append(v)
            ia, ib = divmod(v, nb)
            for da in (-1, 0, 1):
                for db in (-1, 0, 1):
                    ja, jb = ia + da, ib + db
                    if 0 <= ja < na and 0 <= jb < nb:
                        u = ja * nb + jb
                        if front[u] and not seen[u]:
                            seen[u] = True
                            stack.append(u)
        size = len(members)
        if size < prm.min_size:
            continue
        members.sort()
        rows, cols = [v // nb for v in members], [v % nb for v in members]
        sum_a, sum_b = sum(rows), sum(cols)
        ca, cb = sum_a // size, sum_b // size
        rep, rep_d = NONE, None
        best, best_c = NONE, NONE
        for v, ia, ib in zip(members, rows, cols):  # ascending index: a strict < keeps the smallest index on a tie
            d = (ia - ca) ** 2 + (ib - cb) ** 2
            if rep_d is None or d < rep_d:
                rep, rep_d = v, d
            if W is not None and W[v] != NONE and (best == NONE or W[v] < best_c):
                best, best_c = v, W[v]
        for v in members:
            label[v] = len(kept)
        kept.append((seed, size, rep, best, best_c, min(rows), max(rows), min(cols), max(cols), 0, sum_a, sum_b))
    return _result(prm, kept, np.array(label, np.uint32).reshape(na, nb), (sum(free), sum(unknown), sum(front), n_frontiers))


# ------------------------------------------------------------------------------------------------ route (b): whole arrays
def _shift(a, da, db, fill):
    """out[ia, ib] = a[ia + da, ib + db], `fill` where that is outside"""
    na, nb = a.shape
    out = np.full_like(a, fill)
    sa, sb = slice(max(0, -da), na - max(0, da)), slice(max(0, -db), nb - max(0, db))
    ta, tb = slice(max(0, da), na - max(0, -da)), slice(max(0, db), nb - max(0, -db))
    out[sa, sb] = a[ta, tb]
    return out


def frontiers_np(cls, blocked, cost, prm, variant=None):
    assert variant is None or variant in VARIANTS, variant
    na, nb = prm.na, prm.nb
    n = na * nb
    cls = np.asarray(cls, np.uint8).reshape(na, nb)
    k = np.minimum(cls, 31).astype(np.uint32)
    known = cls < 32
    free = known & (((np.uint32(prm.free_mask) >> k) & 1) == 1)
    if blocked is not None and variant != "no_blocked":
        free &= np.asarray(blocked).reshape(na, nb) == 0
    unknown = known & (((np.uint32(prm.unknown_mask) >> k) & 1) == 1)
    edge = [(-1, 0), (1, 0), (0, -1), (0, 1)]
    around = [(da, db) for da in (-1, 0, 1) for db in (-1, 0, 1) if (da, db) != (0, 0)]
    touch = np.zeros((na, nb), bool)
    for da, db in (around if variant == "eight_unknown" else edge):
        touch |= _shift(unknown, da, db, variant == "outside_unknown")
    front = free & touch
    idx = np.arange(n, dtype=np.int64).reshape(na, nb)
    big = np.int64(n)
    L = np.where(front, idx, big)
    links = edge if variant == "four" else around
    while True:
        M = L.copy()
        for da, db in links:
            M = np.minimum(M, _shift(L, da, db, big))
        M = np.where(front, M, big)
        flat = np.append(M.ravel(), big)
        M = flat[M.ravel()].reshape(na, nb)  # the label of my label's cell, itself a member: labels only fall towards the smallest
        if np.array_equal(M, L):
            break
        L = M
    cells = np.flatnonzero(front.ravel())
    roots, inverse, sizes = np.unique(L.ravel()[cells], return_inverse=True, return_counts=True)  # ascending first_cell
    nf = len(roots)
    ia, ib = cells // nb, cells % nb
    sum_a, sum_b = np.zeros(nf, np.int64), np.zeros(nf, np.int64)
    np.add.at(sum_a, inverse, ia)
    np.add.at(sum_b, inverse, ib)
    lo_a, lo_b = np.full(nf, 1 << 20, np.int64), np.full(nf, 1 << 20, np.int64)
    hi_a, hi_b = np.full(nf, -1, np.int64), np.full(nf, -1, np.int64)
    np.minimum.at(lo_a, inverse, ia)
    np.minimum.at(lo_b, inverse, ib)
    np.maximum.at(hi_a, inverse, ia)
    np.maximum.at(hi_b, inverse, ib)
    if variant == "round_centroid":
        ca, cb = (2 * sum_a + sizes) // (2 * sizes), (2 * sum_b + sizes) // (2 * sizes)
    else:
        ca, cb = sum_a // np.maximum(sizes, 1), sum_b // np.maximum(sizes, 1)
    d2 = (ia - ca[inverse]) ** 2 + (ib - cb[inverse]) ** 2
    top = np.uint64(0xFFFFFFFFFFFFFFFF)
    low = lambda c, largest: (NONE - c if largest else c).astype(np.uint64)
    key = np.full(nf, top, np.uint64)
    np.minimum.at(key, inverse, (d2.astype(np.uint64) << np.uint64(32)) | low(cells, variant == "rep_largest"))
    rep = (key & np.uint64(NONE)).astype(np.int64)
    rep = NONE - rep if variant == "rep_largest" else rep
    best, best_c = np.full(nf, NONE, np.int64), np.full(nf, NONE, np.int64)
    if cost is not None:
        w = np.asarray(cost, np.uint32).ravel()[cells].astype(np.int64)
        if variant == "none_smallest":
            order, has = (w + 1) & NONE, np.ones(len(cells), bool)
        else:
            order, has = w, w != NONE
        key = np.full(nf, top, np.uint64)
        np.minimum.at(key, inverse[has], (order[has].astype(np.uint64) << np.uint64(32)) | low(cells[has], variant == "best_largest"))
        got = key != top
        b = (key & np.uint64(NONE)).astype(np.int64)
        b = NONE - b if variant == "best_largest" else b
        best = np.where(got, b, NONE)
        best_c = np.where(got, np.asarray(cost, np.uint32).ravel().astype(np.int64)[np.where(got, b, 0)], NONE)
    keep = sizes > prm.min_size if variant == "gt_min" else sizes >= prm.min_size
    which = np.flatnonzero(keep)
    if variant == "rank_size":
        which = which[np.lexsort((roots[which], -sizes[which]))]
    rank = np.full(nf, NONE, np.int64)
    rank[which] = np.arange(len(which))
    label = np.full(n, NONE, np.uint32)
    label[cells] = rank[inverse]
    kept = [(int(roots[f]), int(sizes[f]), int(rep[f]), int(best[f]), int(best_c[f]), int(lo_a[f]), int(hi_a[f]), int(lo_b[f]), int(hi_b[f]), 0,
             int(sum_a[f]), int(sum_b[f])) for f in which]
    return _result(prm, kept, label.reshape(na, nb), (int(free.sum()), int(unknown.sum()), int(front.sum()), nf))


def same(x, y):
    return x.frontiers.tobytes() == y.frontiers.tobytes() and np.array_equal(x.goal_cells, y.goal_cells) and \
        np.array_equal(x.label, y.label) and tuple(x.counts) == tuple(y.counts)


# ------------------------------------------------------------------------------------------------ cases
def random_case(na, nb, p_unknown, p_obstacle, seed=None, with_blocked=True, with_cost=True, **prm):
    """cls drawn per cell; blocked 2 on OBSTACLE cells and 1 on a seeded twentieth of the LEVEL cells; cost seeded in steps of 16 (so
    that members tie), a quarter of it NONE."""
    rng = np.random.default_rng(1000 * na + nb if seed is None else seed)
    u = rng.random((na, nb))
    cls = np.where(u < p_unknown, UNKNOWN, np.where(u < p_unknown + p_obstacle, OBSTACLE, LEVEL)).astype(np.uint8)
    blocked = np.where(cls == OBSTACLE, 2, np.where((cls == LEVEL) & (rng.random((na, nb)) < 0.05), 1, 0)).astype(np.uint8)
    cost = (rng.integers(0, 64, (na, nb)) * 16).astype(np.uint32)
    cost[rng.random((na, nb)) < 0.25] = NONE
    return Case(cls, blocked if with_blocked else None, cost if with_cost else None, params(cls, **prm))


def serpentine(n=65):
    """Even rows LEVEL, odd rows UNKNOWN but for one LEVEL connector at alternating ends: one frontier under 8-connectivity."""
    cls = np.full((n, n), LEVEL, np.uint8)
    cls[1::2] = UNKNOWN
    for r in range(1, n, 2):
        cls[r, n - 1 if (r // 2) % 2 == 0 else 0] = LEVEL
    return Case(cls, None, None, params(cls, max_frontiers=4))


def diagonal_pairs(n=72):
    """OBSTACLE everywhere; at every corner (8i, 8j), i, j >= 1, two LEVEL cells that touch only diagonally with one UNKNOWN cell
    between them, diagonal and anti-diagonal alternating: 64 frontiers of size 2, 128 under the 4-connected misreading."""
    cls = np.full((n, n), OBSTACLE, np.uint8)
    for i in range(1, n // 8):
        for j in range(1, n // 8):
            a, b = 8 * i, 8 * j
            if (i + j) % 2 == 0:   # (a-1, b-1) and (a, b), UNKNOWN at (a-1, b): an edge neighbour of both
                cls[a - 1, b - 1] = cls[a, b] = LEVEL
                cls[a - 1, b] = UNKNOWN
            else:                  # (a-1, b) and (a, b-1), UNKNOWN at (a, b)
                cls[a - 1, b] = cls[a, b - 1] = LEVEL
                cls[a, b] = UNKNOWN
    return Case(cls, None, None, params(cls, min_size=2, max_frontiers=256))


def constructed():
    """name -> (case, facts): facts["counts"] the seven counts, facts["records"] {rank: {field: value}}, facts["label"] {(ia, ib): rank}"""
    out = {}
    L, U, O = LEVEL, UNKNOWN, OBSTACLE
    g = lambda rows: np.array(rows, np.uint8)
    out["serpentine"] = (serpentine(), {"counts": (2145 + 32, 32 * 64, 2175, 1, 1, 1, 2175), "records": {0: {"first_cell": 0, "size": 2175}}})
    out["diagonal_pairs"] = (diagonal_pairs(), {"counts": (128, 64, 128, 64, 64, 64, 128)})
    cls = np.full((20, 20), L, np.uint8)
    out["all_free"] = (Case(cls, None, None, params(cls)), {"counts": (400, 0, 0, 0, 0, 0, 0)})
    cls = np.full((20, 20), U, np.uint8)
    out["all_unknown"] = (Case(cls, None, None, params(cls)), {"counts": (0, 400, 0, 0, 0, 0, 0)})
    cls = np.full((9, 9), U, np.uint8)
    cls[4, 4] = L
    out["one_free"] = (Case(cls, None, None, params(cls, min_size=1)),
                       {"counts": (1, 80, 1, 1, 1, 1, 1), "records": {0: {"first_cell": 40, "rep_cell": 40, "best_cell": NONE, "best_cost": NONE,
                                                                          "min_a": 4, "max_b": 4, "sum_a": 4, "sum_b": 4}}})
    cls = g([[U, O, O], [O, L, O], [O, O, U]])
    out["diagonal_unknown_only"] = (Case(cls, None, None, params(cls, min_size=1)), {"counts": (1, 2, 0, 0, 0, 0, 0)})
    cls = g([[L, L, L], [L, O, L], [L, L, L]])
    out["edge_no_unknown"] = (Case(cls, None, None, params(cls, min_size=1)), {"counts": (8, 0, 0, 0, 0, 0, 0)})
    cls = g([[L, U, L, O], [L, L, L, O]])
    blocked = g([[0, 0, 1, 2], [0, 0, 0, 2]])
    # (0, 2) touches the UNKNOWN cell but is blocked; (0, 0) and (1, 1) are the frontier, joined diagonally
    out["blocked_alone"] = (Case(cls, blocked, None, params(cls, min_size=1)),
                            {"counts": (4, 1, 2, 1, 1, 1, 2), "label": {(0, 2): NONE, (0, 0): 0, (1, 1): 0}})
    cls = g([[32, 1, 0, 255], [1, 33, 1, 1], [64, 0, 1, 200]])
    out["classes_32_up"] = (Case(cls, None, None, params(cls, min_size=1)), {"counts": (5, 2, 3, 1, 1, 1, 3)})
    cls = g([[5, 7, 5], [9, 5, 31], [5, 31, 5]])
    out["other_masks"] = (Case(cls, None, None, params(cls, free_mask=(1 << 5) | (1 << 9), unknown_mask=(1 << 31) | (1 << 7), min_size=1)),
                          {"counts": (6, 3, 5, 1, 1, 1, 5)})
    # two members at equal distance from the centroid: a row of four frontier cells, centroid column floor(6 / 4) = 1: columns 0 and 2
    # are at d^2 = 1 each, column 1 at 0: no tie there; a row of two (columns 0, 1), centroid 0 -> no tie either.  Three cells
    # (0,0), (0,2), (1,1): centroid (0, 1), d^2 = 1 for all three: the smallest index, cell 0, is the representative.
    cls = g([[L, U, L], [U, L, U], [O, O, O]])
    out["rep_tie"] = (Case(cls, None, None, params(cls, min_size=1)),
                      {"counts": (3, 3, 3, 1, 1, 1, 3), "records": {0: {"rep_cell": 0, "sum_a": 1, "sum_b": 3, "size": 3}}})
    cost = np.array([[7, 0, 5], [0, 5, 0], [0, 0, 0]], np.uint32)
    out["cost_tie"] = (Case(cls, None, cost, params(cls, min_size=1)), {"records": {0: {"best_cell": 2, "best_cost": 5}}})
    cost = np.full((3, 3), NONE, np.uint32)
    cost[1, 0] = 3  # an UNKNOWN cell's cost is nobody's
    out["cost_all_none"] = (Case(cls, None, cost, params(cls, min_size=1)), {"records": {0: {"best_cell": NONE, "best_cost": NONE}}})
    # a frontier of exactly min_size cells and one of min_size - 1
    cls = g([[L, L, L, O, L, L], [U, U, U, O, U, U]])
    out["min_size_exact"] = (Case(cls, None, None, params(cls, min_size=3)),
                             {"counts": (5, 5, 5, 2, 1, 1, 3), "label": {(0, 0): 0, (0, 2): 0, (0, 4): NONE, (0, 5): NONE}})
    return out


def misreading_case():
    """63 x 65 at densities (0.3, 0.1) with blocked and cost, min_size 3: large and small frontiers, ties, cells on the grid's edge."""
    return random_case(63, 65, 0.3, 0.1, seed=7)
