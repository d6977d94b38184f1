"""The ground plan route's contract (include/svo.h, "Ground plan route") restated twice, by two routes that share no code,
both applied to an (na, nb) uint8 `blocked` grid (passable iff 0), an optional (na, nb) uint32 `dist2`, goal and start cell lists:

  route_py   Dijkstra with a heap, cell by cell in Python integers, expanding backwards from the goals; the directions by a loop
             over k = 0 .. 7 per cell and the paths by a walk per start;
  route_np   whole-array Bellman-Ford sweeps in numpy: eight shifted arrays per sweep, repeated until nothing changes; the directions
             by eight whole-array comparisons and the paths by stepping all starts at once.

Neither is the tiled relaxation of the kernels.  Both return a Route: cost (uint32), next (uint8) as (na, nb) arrays, path (n_starts,
max_path) uint32 with NONE where nothing is written, path_len, path_status and the counts (n_goals_used, n_reached, n_unreached,
n_impassable, converged = 1).  `variant` of route_np states one deliberate misreading of the contract each; tests/test_grid_route.py
shows that every one of them changes a result.  Also here: the seeded random cases and the constructed ones with the facts they were
built for.  Nothing here is tuned on the library's output.
"""
import heapq
from collections import namedtuple

import numpy as np

Params = namedtuple("Params", "na nb near_r2 near_weight max_cost max_rounds max_path resume")
Route = namedtuple("Route", "cost next path path_len path_status counts")
Case = namedtuple("Case", "blocked dist2 prm goals starts")
NONE = 0xFFFFFFFF
MAX_COST = 0x7F000000
OK, TRUNCATED, UNREACHED, OUT_OF_GRID, NOT_CONVERGED = range(5)
MOVES = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))  # k = 0 .. 7, raster order of (dia, dib)
VARIANTS = ("corner_cut", "pen_left", "diag5", "four", "tie_largest", "lt_max", "goal_blocked", "none_near", "start_step")
TILES = (16, 32)  # both tile edges the kernels were built with; the shapes below straddle either
SIZES = [(1, 1), (1, 257), (257, 1), (2, 2)] + [(t + d, t + d) for t in TILES for d in (-1, 0, 1)] + \
        [(2 * t + 1, t - 1) for t in TILES] + [(63, 65), (130, 300)]
DENSITIES = (0.05, 0.25, 0.4)
_INF = np.int64(1) << 62


def params(blocked, near_r2=0, near_weight=0, max_cost=MAX_COST, max_rounds=64, max_path=4096, resume=0):
    return Params(blocked.shape[0], blocked.shape[1], near_r2, near_weight, max_cost, max_rounds, max_path, resume)


# ------------------------------------------------------------------------------------------------ route (a): Dijkstra
def route_py(blocked, dist2, prm, goals, starts=()):
    na, nb = prm.na, prm.nb
    n = na * nb
    B = [int(v) != 0 for v in np.asarray(blocked).ravel()]
    D = None if dist2 is None else [int(v) for v in np.asarray(dist2).ravel()]

    def pen(v):
        return prm.near_weight * (prm.near_r2 - D[v]) if D is not None and D[v] < prm.near_r2 else 0

    def moves(v):
        """(k, u, cost of the move v -> u) for every allowed move out of a passable v"""
        ia, ib = divmod(v, nb)
        for k, (da, db) in enumerate(MOVES):
            ja, jb = ia + da, ib + db
            if not (0 <= ja < na and 0 <= jb < nb) or B[ja * nb + jb]:
                continue
            if da and db and (B[ja * nb + ib] or B[ia * nb + jb]):
                continue
            u = ja * nb + jb
            yield k, u, (5 if da == 0 or db == 0 else 7) * (16 + pen(u))

    cost = [NONE] * n
    heap, used = [], 0
    for g in goals:
        g = int(g)
        if g < n and not B[g]:
            used += 1
            if cost[g] != 0:
                cost[g] = 0
                heap.append((0, g))
    heapq.heapify(heap)
    # backwards from the goals: settling u offers cost[u] + (the move v -> u) to every v that may move INTO u.  The allowed moves are
    # symmetric in which pairs they join (the two cells a diagonal passes between are the same either way), the price is not.
    while heap:
        c, u = heapq.heappop(heap)
        if c != cost[u]:
            continue
        pu = pen(u)
        for _, v, _ in moves(u):
            ua, ub = divmod(u, nb)
            va, vb = divmod(v, nb)
            c2 = c + (5 if ua == va or ub == vb else 7) * (16 + pu)
            if c2 <= prm.max_cost and c2 < cost[v]:
                cost[v] = c2
                heapq.heappush(heap, (c2, v))
    nxt = [255] * n
    for v in range(n):
        if cost[v] == 0:
            nxt[v] = 8
        elif cost[v] != NONE:
            for k, u, step in moves(v):
                if cost[u] != NONE and cost[u] + step == cost[v]:
                    nxt[v] = k
                    break
    ns = len(starts)
    path = np.full((ns, prm.max_path if ns else 0), NONE, np.uint32)
    plen, status = np.zeros(ns, np.uint32), np.zeros(ns, np.uint8)
    for i, s in enumerate(starts):
        s = int(s)
        if s >= n:
            status[i] = OUT_OF_GRID
        elif cost[s] == NONE:
            status[i] = UNREACHED
        else:
            cells = [s]
            while nxt[cells[-1]] != 8:
                da, db = MOVES[nxt[cells[-1]]]
                cells.append(cells[-1] + da * nb + db)
            plen[i] = len(cells)
            status[i] = TRUNCATED if len(cells) > prm.max_path else OK
            w = min(len(cells), prm.max_path)
            path[i, :w] = cells[:w]
    closed = sum(B)
    reached = sum(1 for v in range(n) if cost[v] != NONE)
    return Route(np.array(cost, np.uint32).reshape(na, nb), np.array(nxt, np.uint8).reshape(na, nb), path, plen, status,
                 (used, reached, n - closed - reached, closed, 1))


# ------------------------------------------------------------------------------------------------ route (b): numpy sweeps
def _shift(a, da, db, fill):
    """out[ia, ib] = a[ia + da, ib + db], `fill` outside"""
    na, nb = a.shape
    p = np.full((na + 2, nb + 2), fill, a.dtype)
    p[1:-1, 1:-1] = a
    return p[1 + da:1 + da + na, 1 + db:1 + db + nb]


def route_np(blocked, dist2, prm, goals, starts=(), variant=None):
    na, nb = prm.na, prm.nb
    n = na * nb
    assert blocked.shape == (na, nb) and variant in (None,) + VARIANTS
    free = np.asarray(blocked) == 0
    pen = np.zeros((na, nb), np.int64)
    if dist2 is not None:
        d = np.asarray(dist2).astype(np.int64)
        if variant == "none_near":
            d = np.where(d == NONE, 0, d)
        pen = np.where(d < prm.near_r2, prm.near_weight * (prm.near_r2 - d), 0)
    goals = np.asarray(goals, np.int64).ravel()
    ok = goals < n
    ok[ok] &= (free.ravel()[goals[ok]] | (variant == "goal_blocked"))
    cost = np.full(n, _INF, np.int64)
    cost[goals[ok]] = 0
    cost = cost.reshape(na, nb)
    allowed, steps = [], []
    for k, (da, db) in enumerate(MOVES):
        a = free & _shift(free, da, db, False)
        if da and db:
            if variant == "four":
                a = np.zeros_like(a)
            elif variant != "corner_cut":
                a = a & _shift(free, da, 0, False) & _shift(free, 0, db, False)
        w = 5 if da == 0 or db == 0 or variant == "diag5" else 7
        allowed.append(a)
        steps.append(w * (16 + (pen if variant == "pen_left" else _shift(pen, da, db, 0))))
    while True:
        new = cost
        for k, (da, db) in enumerate(MOVES):
            cu = _shift(cost, da, db, _INF)
            cand = np.where(allowed[k] & (cu < _INF), cu + steps[k], _INF)
            within = cand < prm.max_cost if variant == "lt_max" else cand <= prm.max_cost
            new = np.minimum(new, np.where(within, cand, _INF))
        if np.array_equal(new, cost):
            break
        cost = new
    if variant == "start_step":  # the cell's own entering step counted as well
        cost = np.where(cost < _INF, cost + 5 * (16 + pen), _INF)
        cost = np.where(cost <= prm.max_cost, cost, _INF)
    reached = cost < _INF
    nxt = np.full((na, nb), 255, np.uint8)
    order = range(8) if variant == "tie_largest" else range(7, -1, -1)  # the last one written stays
    for k in order:
        da, db = MOVES[k]
        cu = _shift(cost, da, db, _INF)
        nxt[reached & allowed[k] & (cu < _INF) & (cu + steps[k] == cost)] = k
    if variant != "start_step":
        nxt[cost == 0] = 8
    starts = np.asarray(starts, np.int64).ravel()
    ns = len(starts)
    path = np.full((ns, prm.max_path if ns else 0), NONE, np.uint32)
    plen, status = np.zeros(ns, np.uint32), np.zeros(ns, np.uint8)
    inside = starts < n
    status[~inside] = OUT_OF_GRID
    at = np.where(inside, starts, 0)
    live = inside & reached.ravel()[at]
    status[inside & ~live] = UNREACHED
    flat, step_of = nxt.ravel(), np.array([da * nb + db for da, db in MOVES] + [0], np.int64)
    for _ in range(n):
        if not live.any():
            break
        rows = np.flatnonzero(live)
        fits = plen[rows] < prm.max_path
        path[rows[fits], plen[rows[fits]]] = at[rows[fits]]
        plen[rows] += 1
        k = flat[at[rows]]
        live[rows[k >= 8]] = False
        go = rows[k < 8]
        at[go] += step_of[k[k < 8]]
    status[(status == OK) & (plen > prm.max_path)] = TRUNCATED
    closed = int((~free).sum())
    out = np.where(reached, cost, NONE).astype(np.uint32)
    return Route(out, nxt, path, plen, status, (int(ok.sum()), int(reached.sum()), n - closed - int((reached & free).sum()), closed, 1))


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:5], b[:5])) and tuple(a.counts) == tuple(b.counts)


# ------------------------------------------------------------------------------------------------ cases
def random_case(na, nb, density, with_dist2, seed=7):
    """A seeded grid whose impassable bytes take several non-zero values, up to three goals inside it plus one beyond it, a handful of
    starts, and with dist2 seeded values 0 .. 40 under near_r2 = 16, near_weight = 3."""
    rng = np.random.default_rng([seed, na, nb, int(density * 100), int(with_dist2)])
    n = na * nb
    blocked = np.where(rng.random((na, nb)) < density, rng.choice(np.array([1, 2, 255], np.uint8), (na, nb)), 0).astype(np.uint8)
    dist2 = rng.integers(0, 41, (na, nb)).astype(np.uint32) if with_dist2 else None
    goals = np.concatenate([rng.integers(0, n, min(3, n)), [n + 5]]).astype(np.uint32)
    starts = np.concatenate([rng.integers(0, n, min(6, n)), [n], goals[:1]]).astype(np.uint32)
    prm = params(blocked, 16, 3, max_path=64) if with_dist2 else params(blocked, max_path=64)
    return Case(blocked, dist2, prm, goals, starts)


def open_cost(da, db):
    """An open, unweighted grid: min(da, db) diagonals of 7 * 16 and the rest along an axis at 5 * 16, that is
    112 min + 80 (max - min) = 80 max + 32 min."""
    return 80 * max(da, db) + 32 * min(da, db)


def constructed():
    """name -> (Case, facts); facts: "counts" (n_goals_used, n_reached, n_unreached, n_impassable, converged), "cost" {(ia, ib): value},
    "next" {(ia, ib): k}."""
    out = {}
    z = lambda na, nb: np.zeros((na, nb), np.uint8)
    cell = lambda b, ia, ib: ia * b.shape[1] + ib
    # no goal usable: one on an impassable cell, one beyond the grid
    b = z(5, 7)
    b[2, 3] = 1
    b[0, 6] = 200
    out["no_goal_usable"] = (Case(b, None, params(b), [cell(b, 2, 3), 35 + 3], [0]), {"counts": (0, 0, 33, 2, 1), "cost": {(0, 0): NONE}})
    b = np.full((4, 5), 1, np.uint8)
    out["all_blocked"] = (Case(b, None, params(b), [0, 7], [3]), {"counts": (0, 0, 0, 20, 1), "cost": {(1, 2): NONE}, "next": {(0, 0): 255}})
    # a wall with one gap: the gap is entered and left along the axis, since a diagonal would pass between wall cells
    b = z(9, 9)
    b[:, 4] = 1
    b[7, 4] = 0
    out["wall_gap"] = (Case(b, None, params(b), [0], [cell(b, 0, 8)]),
                       {"counts": (1, 73, 0, 8, 1), "cost": {(0, 8): 2 * open_cost(7, 3) + 160, (7, 4): open_cost(7, 3) + 80}, "next": {(7, 5): 3, (7, 4): 3}})
    # rule 2's diagonal: squeezed between two impassable cells it is no move; with one of them open it still is none
    b = np.array([[0, 1], [1, 0]], np.uint8)
    out["squeezed"] = (Case(b, None, params(b), [0], [3]), {"counts": (1, 1, 1, 2, 1), "cost": {(1, 1): NONE}})
    b = np.array([[0, 1], [0, 0]], np.uint8)
    out["half_squeezed"] = (Case(b, None, params(b), [0], [3]), {"counts": (1, 3, 0, 1, 1), "cost": {(1, 1): 160}, "next": {(1, 1): 3, (1, 0): 1}})
    # a goal on a tile's corner, for either tile edge: the four tiles that meet there all see it in the first round
    for t in TILES:
        b = z(t + 8, t + 8)
        out["tile_corner_%d" % t] = (Case(b, None, params(b), [cell(b, t - 1, t - 1)], [0, cell(b, t + 7, t + 7), cell(b, t, 0)]),
                                     {"counts": (1, (t + 8) ** 2, 0, 0, 1),
                                      "cost": {(0, 0): open_cost(t - 1, t - 1), (t + 7, t + 7): open_cost(8, 8), (t, 0): open_cost(1, t - 1), (t, t): 112},
                                      "next": {(t, t): 0, (t - 1, t): 3, (t - 1, t - 1): 8}})
    # two goals at equal cost: the smaller k wins
    b = z(3, 5)
    out["tie"] = (Case(b, None, params(b), [cell(b, 1, 0), cell(b, 1, 4)], [cell(b, 1, 2)]), {"counts": (2, 15, 0, 0, 1), "cost": {(1, 2): 160}, "next": {(1, 2): 3, (0, 2): 3}})
    b = z(3, 3)
    out["tie_diagonal"] = (Case(b, None, params(b), [0, 8], [4]), {"counts": (2, 9, 0, 0, 1), "cost": {(1, 1): 112}, "next": {(1, 1): 0}})
    b = z(2, 4)
    out["duplicate_goal"] = (Case(b, None, params(b), [5, 5, 5], [0]), {"counts": (3, 8, 0, 0, 1), "cost": {(1, 1): 0, (0, 0): 112}})
    # the cap: a cell at exactly max_cost has a cost, one step more has none
    b = z(1, 5)
    out["exact_max_cost"] = (Case(b, None, params(b, max_cost=240), [0], [3, 4]), {"counts": (1, 4, 1, 0, 1), "cost": {(0, 3): 240, (0, 4): NONE}})
    # a corridor of penalised (passable) cells: the way round through the unpenalised row costs 704, the straight one 3 * 80 + 5 * 8080
    b = z(5, 9)
    d = np.full((5, 9), 100, np.uint32)
    d[2, 2:7] = 0
    out["penalty_corridor"] = (Case(b, d, params(b, 16, 100), [cell(b, 2, 0)], [cell(b, 2, 8)]),
                               {"counts": (1, 45, 0, 0, 1), "cost": {(2, 8): 704, (2, 2): 160, (2, 3): 112 + 192}, "next": {(2, 8): 0}})
    # dist2 with NONE entries: they are far, not near
    rng = np.random.default_rng(11)
    b = (rng.random((20, 20)) < 0.15).astype(np.uint8)
    d = rng.integers(0, 30, (20, 20)).astype(np.uint32)
    d[rng.random((20, 20)) < 0.3] = NONE
    b[10, 10] = 0
    out["dist2_none"] = (Case(b, d, params(b, 16, 3), [cell(b, 10, 10)], [0, 399]), {"cost": {(10, 10): 0}})
    return out


def misreading_case():
    """The grid every misreading is shown on ("mixed"): 63 x 65, density 0.25, dist2 seeded 0 .. 40 with a fifth of it NONE, near_r2 16,
    near_weight 3, three goals of which one lies on an impassable cell, and max_cost set to the cost some cell has exactly."""
    rng = np.random.default_rng(23)
    na, nb = 63, 65
    b = np.where(rng.random((na, nb)) < 0.25, 1, 0).astype(np.uint8)
    d = rng.integers(0, 41, (na, nb)).astype(np.uint32)
    d[rng.random((na, nb)) < 0.2] = NONE
    free, closed = np.flatnonzero(b.ravel() == 0), np.flatnonzero(b.ravel() != 0)
    goals = np.array([free[len(free) // 3], free[2 * len(free) // 3], closed[len(closed) // 2]], np.uint32)
    full = route_np(b, d, params(b, 16, 3), goals)
    costs = np.sort(full.cost[full.cost != NONE])
    prm = params(b, 16, 3, max_cost=int(costs[3 * len(costs) // 4]))
    return Case(b, d, prm, goals, np.array([free[0], free[-1]], np.uint32))


def not_converged_case():
    """40 x 200, open, one goal at cell 0: with max_rounds = 1 only the goal's tile and its neighbours run, so cells three or more
    tiles away cannot have a cost yet."""
    b = np.zeros((40, 200), np.uint8)
    return Case(b, None, params(b, max_rounds=1, max_path=256), np.array([0], np.uint32), np.array([199, 40 * 200 - 1, 0], np.uint32))
