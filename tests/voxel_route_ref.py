"""The voxel map route's contract (include/svo.h, "Voxel map route") restated twice, by two routes that share no code, both
applied to a (d2, d1, d0) bool `closed` volume (cell B = j0 + d0 * (j1 + d1 * j2) is its ravel index), an optional (d2, d1, d0)
uint16 `dist2` with 0xFFFF for far, goal and start cell lists:

  route_py   Dijkstra with a heap, cell by cell in Python integers, expanding backwards from the goals; the directions by a loop
             over k = 0 .. 26 per cell and the paths by a walk per start;
  route_np   whole-array Bellman-Ford sweeps in numpy: 26 shifted arrays per sweep, repeated until nothing changes; the directions
             by 26 whole-array comparisons and the paths by stepping all starts at once.

Neither is the tiled relaxation of the kernels.  Both return a Route: cost (uint32), next (uint8) as (d2, d1, d0) arrays, path
(n_starts, max_path) uint32 with NONE where nothing is written, path_len, path_status, the counts (n_goals_used, n_reached,
n_unreached, n_closed, converged = 1) and, from route_np, the number of sweeps that changed a cell.  `variant` of route_np states one
deliberate misreading of the contract each; tests/test_voxel_route.py shows that every one of them changes a result.  Also here: the
bit packing of the occupancy's layout, the seeded random cases and the constructed ones with the facts they were built for.
Nothing here is tuned on the library's output.
"""
import heapq
from collections import namedtuple

import numpy as np

Params = namedtuple("Params", "near_r2 near_weight max_cost max_rounds max_path resume")
Route = namedtuple("Route", "cost next path path_len path_status counts sweeps")
Case = namedtuple("Case", "closed dist2 prm goals starts")
NONE = 0xFFFFFFFF
NONE16 = 0xFFFF
MAX_COST = 0x7F000000
SELF, NO_MOVE = 13, 255
OK, TRUNCATED, UNREACHED, OUT_OF_VOLUME, NOT_CONVERGED = range(5)
# k = 9 (dj2 + 1) + 3 (dj1 + 1) + (dj0 + 1); MOVES[k] = (dj0, dj1, dj2)
MOVES = tuple((k % 3 - 1, k // 3 % 3 - 1, k // 9 - 1) for k in range(27))
VARIANTS = ("corner_cut", "vertex_faces", "pen_left", "w577", "w345", "six", "eighteen", "tie_largest", "lt_max", "goal_closed", "none_near",
            "swap12", "row_wrap")
TILES = ((8, 8, 8), (16, 8, 4))  # both tile shapes the kernels were built with; the shapes below straddle the edges of either
# (d0, d1, d2): d0 a multiple of 64; d1 and d2 one below, at and one above every tile edge (4, 8, 16) and its double, 1, and 33
SIZES = [(64, 1, 1), (64, 3, 1), (64, 7, 3), (64, 8, 4), (64, 9, 5), (64, 4, 7), (64, 5, 8), (64, 15, 9), (64, 16, 3), (64, 17, 9),
         (64, 3, 15), (64, 4, 16), (64, 5, 17), (128, 17, 1), (64, 33, 1), (64, 1, 17), (128, 33, 17)]
DENSITIES = (0.05, 0.25, 0.4)
_INF = np.int64(1) << 62


def params(near_r2=0, near_weight=0, max_cost=MAX_COST, max_rounds=64, max_path=4096, resume=0):
    return Params(near_r2, near_weight, max_cost, max_rounds, max_path, resume)


def dims_of(closed):
    return (closed.shape[2], closed.shape[1], closed.shape[0])


def pack(closed):
    """The occupancy's layout: bit B & 63 of uint64 word B >> 6."""
    flat = np.asarray(closed, bool).ravel()
    assert flat.size % 64 == 0
    return np.packbits(flat, bitorder="little").view(np.uint64)


def unpack(words, dims):
    bits = np.unpackbits(np.asarray(words, np.uint64).view(np.uint8), bitorder="little").astype(bool)
    return bits.reshape(dims[2], dims[1], dims[0])


def cell(closed, j0, j1, j2):
    return j0 + closed.shape[2] * (j1 + closed.shape[1] * j2)


# ------------------------------------------------------------------------------------------------ route (a): Dijkstra
def route_py(closed, dist2, prm, goals, starts=()):
    d2_, d1_, d0_ = closed.shape
    n = d0_ * d1_ * d2_
    B = [bool(v) for v in np.asarray(closed).ravel()]
    D = None if dist2 is None else [int(v) for v in np.asarray(dist2).ravel()]
    unit = [16] * n
    if D is not None:
        for v in range(n):
            if D[v] != NONE16 and D[v] < prm.near_r2:
                unit[v] = 16 + prm.near_weight * (prm.near_r2 - D[v])
    # per move: its weight, and the offsets of the box's cells other than the cell moved out of
    box = []
    for k, (a, b, c) in enumerate(MOVES):
        if k == SELF:
            box.append(None)
            continue
        cells = [(x, y, z) for x in {0, a} for y in {0, b} for z in {0, c} if (x, y, z) != (0, 0, 0)]
        box.append((3 + 2 * (abs(a) + abs(b) + abs(c)), cells))

    def moves(v):
        """(k, u, w) for every allowed move out of the passable cell v"""
        j0 = v % d0_
        j1 = v // d0_ % d1_
        j2 = v // (d0_ * d1_)
        for k in range(27):
            if k == SELF:
                continue
            a, b, c = MOVES[k]
            if not (0 <= j0 + a < d0_ and 0 <= j1 + b < d1_ and 0 <= j2 + c < d2_):
                continue
            w, cells = box[k]
            for x, y, z in cells:
                if B[v + x + d0_ * (y + d1_ * z)]:
                    break
            else:
                yield k, v + a + d0_ * (b + d1_ * c), w

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
    # symmetric in which pairs they join (the box is the same either way), the price, that of the cell entered, is not.
    while heap:
        c, u = heapq.heappop(heap)
        if c != cost[u]:
            continue
        for _, v, w in moves(u):
            c2 = c + w * unit[u]
            if c2 <= prm.max_cost and c2 < cost[v]:
                cost[v] = c2
                heapq.heappush(heap, (c2, v))
    nxt = [NO_MOVE] * n
    for v in range(n):
        if cost[v] == 0:
            nxt[v] = SELF
        elif cost[v] != NONE:
            for k, u, w in moves(v):
                if cost[u] != NONE and cost[u] + w * unit[u] == cost[v]:
                    nxt[v] = k
                    break
    ns = len(starts)
    path = np.full((ns, prm.max_path if ns else 0), NONE, np.uint32)
    plen, status = np.zeros(ns, np.uint32), np.zeros(ns, np.uint8)
    for i, s in enumerate(starts):
        s = int(s)
        if s >= n:
            status[i] = OUT_OF_VOLUME
        elif cost[s] == NONE:
            status[i] = UNREACHED
        else:
            cells = [s]
            while nxt[cells[-1]] != SELF:
                a, b, c = MOVES[nxt[cells[-1]]]
                cells.append(cells[-1] + a + d0_ * (b + d1_ * c))
            plen[i] = len(cells)
            status[i] = TRUNCATED if len(cells) > prm.max_path else OK
            w = min(len(cells), prm.max_path)
            path[i, :w] = cells[:w]
    n_closed = sum(B)
    reached = sum(1 for v in range(n) if cost[v] != NONE)
    return Route(np.array(cost, np.uint32).reshape(closed.shape), np.array(nxt, np.uint8).reshape(closed.shape), path, plen, status,
                 (used, reached, n - n_closed - reached, n_closed, 1), None)


# ------------------------------------------------------------------------------------------------ route (b): numpy sweeps
def _shift(a, mv, fill, wrap=False):
    """out[j2, j1, j0] = a[j2 + dj2, j1 + dj1, j0 + dj0], `fill` outside.  wrap (a misreading): axis 0 is stepped in the ravel index,
    so that it runs on from the end of one row into the next."""
    a0, a1, a2 = mv
    d2_, d1_, d0_ = a.shape
    p = np.full((d2_ + 2, d1_ + 2, d0_ + 2), fill, a.dtype)
    p[1:-1, 1:-1, 1:-1] = a
    if not wrap:
        return p[1 + a2:1 + a2 + d2_, 1 + a1:1 + a1 + d1_, 1 + a0:1 + a0 + d0_]
    s = p[1 + a2:1 + a2 + d2_, 1 + a1:1 + a1 + d1_, 1:-1].ravel()
    f = np.concatenate([np.full(1, fill, a.dtype), s, np.full(1, fill, a.dtype)])
    return f[1 + a0:1 + a0 + s.size].reshape(a.shape)


def route_np(closed, dist2, prm, goals, starts=(), variant=None):
    assert variant in (None,) + VARIANTS
    closed = np.asarray(closed, bool)
    d2_, d1_, d0_ = closed.shape
    n = closed.size
    wrap = variant == "row_wrap"
    free = ~closed
    pen = np.zeros(closed.shape, np.int64)
    if dist2 is not None:
        d = np.asarray(dist2).astype(np.int64)
        d = np.where(d == NONE16, 0 if variant == "none_near" else _INF, d)
        pen = np.where(d < prm.near_r2, prm.near_weight * (prm.near_r2 - d), 0)
    goals = np.asarray(goals, np.int64).ravel()
    if variant == "swap12":  # the cell number read as j0 + d0 * (j2 + d2 * j1)
        j0, r = goals % d0_, goals // d0_
        j2, j1 = r % d2_, r // d2_
        goals = np.where(j1 < d1_, j0 + d0_ * (j1 + d1_ * j2), n)
    ok = goals < n
    ok[ok] &= (free.ravel()[goals[ok]] | (variant == "goal_closed"))
    cost = np.full(n, _INF, np.int64)
    cost[goals[ok]] = 0
    cost = cost.reshape(closed.shape)
    weights = {None: (5, 7, 9), "w577": (5, 7, 7), "w345": (3, 4, 5)}.get(variant, (5, 7, 9))
    allowed, steps = {}, {}
    for k, mv in enumerate(MOVES):
        if k == SELF:
            continue
        changed = sum(1 for v in mv if v)
        a = free & _shift(free, mv, False, wrap)
        if (variant == "six" and changed > 1) or (variant == "eighteen" and changed > 2):
            a = np.zeros_like(a)
        between = [(x, y, z) for x in {0, mv[0]} for y in {0, mv[1]} for z in {0, mv[2]} if (x, y, z) not in ((0, 0, 0), mv)]
        if changed == 2 and variant == "corner_cut":
            between = []
        if changed == 3 and variant == "vertex_faces":
            between = [m for m in between if sum(1 for v in m if v) == 1]
        for m in between:
            a = a & _shift(free, m, False, wrap)
        allowed[k] = a
        steps[k] = weights[changed - 1] * (16 + (pen if variant == "pen_left" else _shift(pen, mv, 0, wrap)))
    sweeps = 0
    while True:
        new = cost
        for k, mv in enumerate(MOVES):
            if k == SELF:
                continue
            cu = _shift(cost, mv, _INF, wrap)
            cand = np.where(allowed[k] & (cu < _INF), cu + steps[k], _INF)
            within = cand < prm.max_cost if variant == "lt_max" else cand <= prm.max_cost
            new = np.minimum(new, np.where(within, cand, _INF))
        if np.array_equal(new, cost):
            break
        cost = new
        sweeps += 1
    reached = cost < _INF
    nxt = np.full(closed.shape, NO_MOVE, np.uint8)
    order = range(27) if variant == "tie_largest" else range(26, -1, -1)  # the last one written stays
    for k in order:
        if k == SELF:
            continue
        cu = _shift(cost, MOVES[k], _INF, wrap)
        nxt[reached & allowed[k] & (cu < _INF) & (cu + steps[k] == cost)] = k
    nxt[cost == 0] = SELF
    starts = np.asarray(starts, np.int64).ravel()
    ns = len(starts)
    path = np.full((ns, prm.max_path if ns else 0), NONE, np.uint32)
    plen, status = np.zeros(ns, np.uint32), np.zeros(ns, np.uint8)
    inside = starts < n
    status[~inside] = OUT_OF_VOLUME
    at = np.where(inside, starts, 0)
    live = inside & reached.ravel()[at]
    status[inside & ~live] = UNREACHED
    flat, step_of = nxt.ravel(), np.array([a + d0_ * (b + d1_ * c) for a, b, c in MOVES], np.int64)
    for _ in range(n):
        if not live.any():
            break
        rows = np.flatnonzero(live)
        fits = plen[rows] < prm.max_path
        path[rows[fits], plen[rows[fits]]] = at[rows[fits]]
        plen[rows] += 1
        k = flat[at[rows]]
        stop = (k == SELF) | (k == NO_MOVE)
        live[rows[stop]] = False
        at[rows[~stop]] += step_of[k[~stop]]
    status[(status == OK) & (plen > prm.max_path)] = TRUNCATED
    n_closed = int(closed.sum())
    out = np.where(reached, cost, NONE).astype(np.uint32)
    return Route(out, nxt, path, plen, status, (int(ok.sum()), int(reached.sum()), n - n_closed - int((reached & free).sum()), n_closed, 1), sweeps)


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:5], b[:5])) and tuple(a.counts) == tuple(b.counts)


# ------------------------------------------------------------------------------------------------ cases
def random_case(dims, density, with_dist2, seed=7):
    """A seeded volume, two goals anywhere inside it, one on a passable cell and one beyond the volume, a handful of starts, paths of
    up to 24 cells, and with dist2 seeded values 0 .. 40, a tenth of them 0xFFFF, under near_r2 = 16, near_weight = 3."""
    d0_, d1_, d2_ = dims
    rng = np.random.default_rng([seed, d0_, d1_, d2_, int(density * 100), int(with_dist2)])
    n = d0_ * d1_ * d2_
    closed = rng.random((d2_, d1_, d0_)) < density
    dist2 = None
    if with_dist2:
        dist2 = rng.integers(0, 41, closed.shape).astype(np.uint16)
        dist2[rng.random(closed.shape) < 0.1] = NONE16
    free = np.flatnonzero(~closed.ravel())
    goals = np.concatenate([rng.integers(0, n, 2), free[rng.integers(0, len(free), 1)], [n + 5]]).astype(np.uint32)
    starts = np.concatenate([rng.integers(0, n, 6), [n], goals[2:3]]).astype(np.uint32)
    prm = params(16, 3, max_path=24) if with_dist2 else params(max_path=24)
    return Case(closed, dist2, prm, goals, starts)


def open_cost(da, db, dc):
    """An open, unweighted volume: with the differences sorted a >= b >= c, c vertex moves (9 * 16), b - c edge moves (7 * 16) and
    a - b face moves (5 * 16): 144 c + 112 (b - c) + 80 (a - b) = 80 a + 32 b + 32 c."""
    a, b, c = sorted((da, db, dc), reverse=True)
    return 80 * a + 32 * b + 32 * c


def constructed():
    """name -> (Case, facts); facts: "counts" (n_goals_used, n_reached, n_unreached, n_closed, converged), "cost" {(j0, j1, j2): value},
    "next" {(j0, j1, j2): k}, "status" [per start]."""
    out = {}
    z = lambda d0_, d1_, d2_: np.zeros((d2_, d1_, d0_), bool)
    # no goal usable: one on a closed cell, one beyond the volume
    c = z(64, 3, 2)
    c[1, 2, 3] = True
    c[0, 0, 6] = True
    out["no_goal_usable"] = (Case(c, None, params(), [cell(c, 3, 2, 1), 64 * 3 * 2 + 3], [0]),
                             {"counts": (0, 0, 382, 2, 1), "cost": {(0, 0, 0): NONE}, "status": [UNREACHED]})
    c = np.ones((2, 2, 64), bool)
    out["all_closed"] = (Case(c, None, params(), [0, 7], [3]), {"counts": (0, 0, 0, 256, 1), "cost": {(1, 1, 1): NONE}, "next": {(0, 0, 0): NO_MOVE}, "status": [UNREACHED]})
    # a slab across axis 2 with one hole: the hole is entered and left along axis 2, since every edge or vertex move through the
    # slab's layer would pass between slab cells
    c = z(64, 9, 9)
    c[4, :, :] = True
    c[4, 7, 5] = False
    far = open_cost(5, 7, 3)  # from (0, 0, 0) to the cell under the hole, (5, 7, 3)
    out["slab_hole"] = (Case(c, None, params(), [0], [cell(c, 0, 0, 8)]),
                        {"counts": (1, 64 * 9 * 9 - 64 * 9 + 1, 0, 64 * 9 - 1, 1),
                         "cost": {(5, 7, 3): far, (5, 7, 4): far + 80, (5, 7, 5): far + 160, (0, 0, 8): far + 160 + open_cost(5, 7, 3)},
                         "next": {(5, 7, 5): 4, (5, 7, 4): 4}, "status": [OK]})
    # rule 2's vertex move: with the three face cells closed it is no move, and the goal cannot be reached at all
    c = z(64, 2, 2)
    c[:, :, 2:] = True
    for m in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        c[m[2], m[1], m[0]] = True
    out["vertex_squeezed"] = (Case(c, None, params(), [0], [cell(c, 1, 1, 1)]), {"counts": (1, 1, 4, 251, 1), "cost": {(1, 1, 1): NONE}, "status": [UNREACHED]})
    # ... with only the three edge cells closed the vertex move is none either, and so is every face and edge move into the far corner
    c = z(64, 2, 2)
    c[:, :, 2:] = True
    for m in ((1, 1, 0), (1, 0, 1), (0, 1, 1)):
        c[m[2], m[1], m[0]] = True
    out["vertex_edges_closed"] = (Case(c, None, params(), [0], [cell(c, 1, 1, 1)]), {"counts": (1, 4, 1, 251, 1), "cost": {(1, 1, 1): NONE, (1, 0, 0): 80}, "status": [UNREACHED]})
    # an edge move between two closed cells is none: the way round over the third axis is a face move up, the same edge move in the
    # open layer and a face move down (the edge and vertex moves that would shorten it pass a closed cell each)
    c = z(64, 2, 2)
    c[:, :, 2:] = True
    c[0, 0, 1] = c[0, 1, 0] = True
    out["edge_squeezed"] = (Case(c, None, params(), [0], [cell(c, 1, 1, 0)]),
                            {"counts": (1, 6, 0, 250, 1), "cost": {(1, 1, 0): 80 + 112 + 80, (1, 1, 1): 112 + 80, (0, 0, 1): 80}, "next": {(1, 1, 0): cell_code(0, 0, 1)},
                             "status": [OK]})
    # the no-wrap rule: a goal in the last cell of a row and a start in the first cell of the next are 63 cells apart, not one
    c = z(64, 2, 1)
    out["no_wrap"] = (Case(c, None, params(), [63], [64]), {"counts": (1, 128, 0, 0, 1), "cost": {(0, 1, 0): open_cost(63, 1, 0), (63, 1, 0): 80}, "status": [OK]})
    c = z(64, 2, 2)
    out["duplicate_goal"] = (Case(c, None, params(), [65, 65, 65], [0]), {"counts": (3, 256, 0, 0, 1), "cost": {(1, 1, 0): 0, (0, 0, 0): 112, (0, 0, 1): 144}, "status": [OK]})
    # starts outside the volume and on closed cells, and one cell per path
    c = z(64, 3, 3)
    c[1, 1, 5] = True
    out["starts_and_max_path_1"] = (Case(c, None, params(max_path=1), [0], [64 * 9, 0xFFFFFFFF, cell(c, 5, 1, 1), 0, cell(c, 9, 2, 2)]),
                                    {"counts": (1, 64 * 9 - 1, 0, 1, 1), "status": [OUT_OF_VOLUME, OUT_OF_VOLUME, UNREACHED, OK, TRUNCATED]})
    # the cap: a cell at exactly max_cost has a cost, one step more has none
    c = z(64, 1, 1)
    out["exact_max_cost"] = (Case(c, None, params(max_cost=240), [0], [3, 4]), {"counts": (1, 4, 60, 0, 1), "cost": {(3, 0, 0): 240, (4, 0, 0): NONE}, "status": [OK, UNREACHED]})
    # ties: the smallest k wins
    c = z(64, 3, 3)
    out["tie"] = (Case(c, None, params(), [cell(c, 0, 0, 0), cell(c, 2, 2, 2), cell(c, 2, 0, 0)], [cell(c, 1, 1, 1)]),
                  {"cost": {(1, 1, 1): 144, (1, 0, 0): 80}, "next": {(1, 1, 1): 0, (1, 0, 0): 12}, "status": [OK]})
    # a corridor of penalised (passable) cells along axis 0 in a one-layer volume: the way round through the unpenalised row wins
    c = z(64, 5, 1)
    c[:, :, 9:] = True
    d = np.full(c.shape, 100, np.uint16)
    d[0, 2, 2:7] = 0
    out["penalty_corridor"] = (Case(c, d, params(16, 100), [cell(c, 0, 2, 0)], [cell(c, 8, 2, 0)]),
                               {"cost": {(8, 2, 0): 704, (2, 2, 0): 160, (3, 2, 0): 112 + 192}, "status": [OK]})
    return out


def cell_code(a, b, c):
    return 9 * (c + 1) + 3 * (b + 1) + (a + 1)


def misreading_case():
    """The volume every misreading is shown on ("mixed"): 64 x 17 x 9, density 0.25, dist2 seeded 0 .. 40 with a fifth of it 0xFFFF,
    near_r2 16, near_weight 3, three goals of which one lies on a closed cell, and max_cost set to the cost the cell at the upper
    quartile of the uncapped field has."""
    rng = np.random.default_rng(23)
    shape = (9, 17, 64)
    c = rng.random(shape) < 0.25
    d = rng.integers(0, 41, shape).astype(np.uint16)
    d[rng.random(shape) < 0.2] = NONE16
    free, shut = np.flatnonzero(~c.ravel()), np.flatnonzero(c.ravel())
    goals = np.array([free[len(free) // 3], free[2 * len(free) // 3], shut[len(shut) // 2]], np.uint32)
    full = route_np(c, d, params(16, 3), goals)
    costs = np.sort(full.cost[full.cost != NONE])
    prm = params(16, 3, max_cost=int(costs[3 * len(costs) // 4]))
    return Case(c, d, prm, goals, np.array([free[0], free[-1]], np.uint32))


def serpentine_case():
    """128 x 8 x 17, slabs across axis 2 at every other layer, each with a hole column at alternating ends of axis 0: the only way from
    the goal in layer 0 to layer 16 runs the volume's length eight times, more than three tiles of either shape each time.  With
    max_rounds = 1 nothing beyond the goal's tile and its neighbours can have a cost."""
    c = np.zeros((17, 8, 128), bool)
    for i, j2 in enumerate(range(1, 17, 2)):
        c[j2, :, :] = True
        c[j2, :, 127 if i % 2 == 0 else 0] = False
    return Case(c, None, params(max_rounds=1, max_path=2048), np.array([0], np.uint32), np.array([cell(c, 0, 0, 16), cell(c, 127, 7, 16), 0], np.uint32))
