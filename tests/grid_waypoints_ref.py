"""The ground plan waypoints' contract (include/svo.h, "Ground plan waypoints") restated twice, by two routes that share no
code, both applied to an (na, nb) uint8 `blocked` grid (passable iff 0), an optional (na, nb) uint32 `dist2` and a route's path,
path_len and path_status:

  waypoints_py   plain Python integers: SOLID cell by cell, rule 3's line step by step from the closed formula, CLEAR by a loop over
                 the steps, the greedy of rule 5 in index order, the length by math.sqrt;
  waypoints_np   whole arrays in numpy: every L_i of every pair (k, j) of a path at once, CLEAR for all pairs as one boolean matrix,
                 then the chain over that matrix.

Neither is the kernel's form (one candidate per thread, remainders instead of the closed formula, early exit).  Both return a Way: way
and way_index (n_paths, max_way) uint32 with `fill` where nothing is written, way_len, way_status, length (float64) and the counts
(n_used, n_skipped, n_cells_in, n_waypoints, n_forced, n_full, max_d2).  `variant` of waypoints_np states one deliberate misreading of
the contract each; tests/test_grid_waypoints.py shows that every one of them changes a result on a committed input.  Also here: the
seeded cases.  Nothing here is tuned on the library's output.
"""
import math
from collections import namedtuple

import numpy as np

import grid_route_ref as R

Params = namedtuple("Params", "na nb path_stride max_look min_dist2 max_way cell_size")
Case = namedtuple("Case", "blocked dist2 path path_len path_status prm")
Way = namedtuple("Way", "way way_index way_len way_status length counts")
NONE = 0xFFFFFFFF
OK, PATH_TRUNCATED, FULL, SKIPPED, BAD_CELL = 0, 1, 2, 4, 5
VARIANTS = ("first_failure", "swapped_ends", "both_sides_corner", "open_ends", "euclid_look", "no_index_limit", "dist2_le",
            "forced_uncounted", "length_written", "tie_towards")


def _why_skipped(status, m, entries, n):
    """rule 2: 0 for a used path, else SKIPPED or BAD_CELL"""
    if status is not None and int(status) not in (R.OK, R.TRUNCATED):
        return SKIPPED
    if m < 1:
        return SKIPPED
    return BAD_CELL if any(int(c) >= n for c in entries) else 0


def _empty(n_paths, prm, fill):
    return (np.full((n_paths, prm.max_way), fill, np.uint32), np.full((n_paths, prm.max_way), fill, np.uint32), np.zeros(n_paths, np.uint32),
            np.zeros(n_paths, np.uint8), np.zeros(n_paths, np.float64))


# ------------------------------------------------------------------------------------------------ route (a): plain loops
def line_py(va, vb, ta, tb):
    """rule 3: [L_0, ..., L_n]"""
    da, db = ta - va, tb - vb
    n = max(abs(da), abs(db))
    sa, sb = (da > 0) - (da < 0), (db > 0) - (db < 0)
    if n == 0:
        return [(va, vb)]
    return [(va + sa * ((2 * i * abs(da) + n) // (2 * n)), vb + sb * ((2 * i * abs(db) + n) // (2 * n))) for i in range(n + 1)]


def clear_py(solid, V, T, max_look):
    """rule 4 over solid(ia, ib)"""
    L = line_py(*V, *T)
    n = len(L) - 1
    if n > max_look or solid(*V) or solid(*T):
        return False
    for i in range(1, n + 1):
        (pa, pb), (qa, qb) = L[i - 1], L[i]
        if qa != pa and qb != pb and (solid(qa, pb) or solid(pa, qb)):
            return False
        if i < n and solid(qa, qb):
            return False
    return True


def waypoints_py(blocked, dist2, path, path_len, path_status, prm, fill=NONE):
    na, nb, n = prm.na, prm.nb, prm.na * prm.nb
    B = [[int(v) for v in row] for row in np.asarray(blocked)]
    D = None if dist2 is None else [[int(v) for v in row] for row in np.asarray(dist2)]

    def solid(ia, ib):
        return B[ia][ib] != 0 or (D is not None and D[ia][ib] < prm.min_dist2)

    n_paths = len(path_len)
    way, index, wlen, status, length = _empty(n_paths, prm, fill)
    used = skipped = cells_in = waypoints = forced = full = max_d2 = 0
    for p in range(n_paths):
        m = min(int(path_len[p]), prm.path_stride)
        cells = [int(c) for c in path[p, :m]]
        why = _why_skipped(None if path_status is None else path_status[p], m, cells, n)
        if why:
            status[p] = why
            skipped += 1
            continue
        at = [divmod(c, nb) for c in cells]
        ks = [0]
        while ks[-1] < m - 1:
            k = ks[-1]
            best = None
            for j in range(k + 2, min(k + prm.max_look, m - 1) + 1):
                if clear_py(solid, at[k], at[j], prm.max_look):
                    best = j  # the largest clear j: the loop does not stop at a failure
            if best is None:
                best = k + 1
                forced += 0 if clear_py(solid, at[k], at[k + 1], prm.max_look) else 1
            ks.append(best)
        w = len(ks)
        s = 0.0
        for t in range(1, w):
            (a0, b0), (a1, b1) = at[ks[t - 1]], at[ks[t]]
            d2 = (a1 - a0) ** 2 + (b1 - b0) ** 2
            max_d2 = max(max_d2, d2)
            s = s + math.sqrt(float(d2))
        for t in range(min(w, prm.max_way)):
            way[p, t], index[p, t] = cells[ks[t]], ks[t]
        wlen[p], length[p] = w, s * prm.cell_size
        status[p] = (PATH_TRUNCATED if int(path_len[p]) > prm.path_stride else 0) | (FULL if w > prm.max_way else 0)
        used, cells_in, waypoints, full = used + 1, cells_in + m, waypoints + w, full + (w > prm.max_way)
    return Way(way, index, wlen, status, length, (used, skipped, cells_in, waypoints, forced, full, max_d2))


# ------------------------------------------------------------------------------------------------ route (b): whole arrays
def solid_np(blocked, dist2, prm, variant=None):
    s = np.asarray(blocked) != 0
    if dist2 is not None:
        d = np.asarray(dist2).astype(np.int64)
        s = s | ((d <= prm.min_dist2) if variant == "dist2_le" else (d < prm.min_dist2))
    return s


def clear_matrix_np(solid, cells, prm, variant=None, width=None):
    """C[k, d - 1] = CLEAR(path[k], path[k + d]) for d = 1 .. width (max_look unless told), False where k + d is past the path."""
    nb, L = prm.nb, prm.max_look
    m = len(cells)
    width = L if width is None else width
    a, b = (np.asarray(cells, np.int64) // nb).astype(np.int32), (np.asarray(cells, np.int64) % nb).astype(np.int32)
    out = np.zeros((m, width), bool)
    rows = max(1, (1 << 21) // max(1, width * (L + 1)))
    for k0 in range(0, m, rows):
        k = np.arange(k0, min(k0 + rows, m))[:, None]
        j = k + np.arange(1, width + 1)[None, :]
        valid = j < m
        jj = np.minimum(j, m - 1)
        va, vb, ta, tb = a[k], b[k], a[jj], b[jj]
        if variant == "swapped_ends":
            va, vb, ta, tb = np.broadcast_to(ta, jj.shape), np.broadcast_to(tb, jj.shape), np.broadcast_to(va, jj.shape), np.broadcast_to(vb, jj.shape)
        else:
            va, vb = np.broadcast_to(va, jj.shape), np.broadcast_to(vb, jj.shape)
        da, db = ta - va, tb - vb
        n = np.maximum(np.abs(da), np.abs(db))
        near = (da * da + db * db <= L * L) if variant == "euclid_look" else (n <= L)
        ok = valid & near
        if variant != "open_ends":
            ok = ok & ~solid[va, vb] & ~solid[ta, tb]
        nc = np.minimum(n, L)  # pairs beyond the look are refused already; their lines are not drawn
        i = np.minimum(np.arange(0, L + 1, dtype=np.int32)[None, None, :], nc[:, :, None])  # steps past n repeat L_n
        n2 = 2 * np.maximum(nc, 1)[:, :, None]
        half = n2 // 2 - (1 if variant == "tie_towards" else 0)
        scale = np.where(n <= L, 1, 0)[:, :, None]  # keeps the offsets of a refused pair at 0, inside the grid
        pa = scale * ((2 * i * np.abs(da)[:, :, None] + half) // n2)
        pb = scale * ((2 * i * np.abs(db)[:, :, None] + half) // n2)
        la, lb = va[:, :, None] + np.sign(da)[:, :, None] * pa, vb[:, :, None] + np.sign(db)[:, :, None] * pb
        step = np.arange(0, L + 1)[None, None, :]
        interior = (step >= 1) & (step <= nc[:, :, None] - 1)
        ok = ok & ~(solid[la, lb] & interior).any(axis=2)
        qa, qb, ra, rb = la[:, :, 1:], lb[:, :, 1:], la[:, :, :-1], lb[:, :, :-1]  # L_i and L_(i-1)
        diagonal = (qa != ra) & (qb != rb)
        s1, s2 = solid[qa, rb], solid[ra, qb]
        shut = (s1 & s2) if variant == "both_sides_corner" else (s1 | s2)
        ok = ok & ~(diagonal & shut).any(axis=2)
        out[k[:, 0]] = ok
    return out


def waypoints_np(blocked, dist2, path, path_len, path_status, prm, fill=NONE, variant=None):
    assert variant in (None,) + VARIANTS and np.asarray(blocked).shape == (prm.na, prm.nb)
    n = prm.na * prm.nb
    solid = solid_np(blocked, dist2, prm, variant)
    n_paths = len(path_len)
    way, index, wlen, status, length = _empty(n_paths, prm, fill)
    path = np.asarray(path)
    m_all = np.minimum(np.asarray(path_len).astype(np.int64), prm.path_stride)
    used = skipped = cells_in = waypoints = forced = full = max_d2 = 0
    for p in range(n_paths):
        m = int(m_all[p])
        cells = path[p, :m].astype(np.int64)
        why = _why_skipped(None if path_status is None else path_status[p], m, cells, n)
        if why:
            status[p] = why
            skipped += 1
            continue
        reach = max(m - 1, 1) if variant == "no_index_limit" else prm.max_look
        C = clear_matrix_np(solid, cells, prm, variant, reach)
        ks = [0]
        while ks[-1] < m - 1:
            k = ks[-1]
            far = C[k, 1:]  # d = 2 ..
            if variant == "first_failure":
                far = np.logical_and.accumulate(far)
            d = np.flatnonzero(far)
            if len(d):
                ks.append(k + 2 + int(d[-1]))
            else:
                ks.append(k + 1)
                forced += 0 if C[k, 0] or variant == "forced_uncounted" else 1
        ks = np.array(ks, np.int64)
        w = len(ks)
        a, b = cells[ks] // prm.nb, cells[ks] % prm.nb
        d2 = np.diff(a) ** 2 + np.diff(b) ** 2
        if w > 1:
            max_d2 = max(max_d2, int(d2.max()))
        counted = d2[:max(prm.max_way - 1, 0)] if variant == "length_written" else d2
        s = np.add.accumulate(np.sqrt(counted.astype(np.float64)))  # in order
        keep = min(w, prm.max_way)
        way[p, :keep], index[p, :keep] = cells[ks[:keep]], ks[:keep]
        wlen[p], length[p] = w, (float(s[-1]) if len(s) else 0.0) * prm.cell_size
        status[p] = (PATH_TRUNCATED if int(path_len[p]) > prm.path_stride else 0) | (FULL if w > prm.max_way else 0)
        used, cells_in, waypoints, full = used + 1, cells_in + m, waypoints + w, full + (w > prm.max_way)
    return Way(way, index, wlen, status, length, (used, skipped, cells_in, waypoints, forced, full, max_d2))


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a.length.tobytes() == b.length.tobytes() and tuple(a.counts) == tuple(b.counts)


# ------------------------------------------------------------------------------------------------ cases
DENSITIES = (0.05, 0.18, 0.3)


def dist2_brute(blocked, max_dist=64):
    """The clearance's dist2 of a small grid whose sources are the impassable cells, by all pairs."""
    na, nb = blocked.shape
    src = np.argwhere(blocked != 0)
    if len(src) == 0:
        return np.full((na, nb), NONE, np.uint32)
    ia, ib = np.meshgrid(np.arange(na), np.arange(nb), indexing="ij")
    d = ((ia[:, :, None] - src[:, 0]) ** 2 + (ib[:, :, None] - src[:, 1]) ** 2).min(axis=2)
    return np.where(d <= max_dist * max_dist, d, NONE).astype(np.uint32)


def route_case(na, nb, density, n_paths, max_look, seed=7, max_path=None, with_dist2=False, min_dist2=0, max_way=64, foreign=0.0, cell_size=0.25,
               router=None):
    """A seeded grid, one goal, n_paths starts anywhere in it (some on impassable cells, some cut off: every route status but
    NOT_CONVERGED where the grid allows), the paths by tests/grid_route_ref.py's route over that grid.  foreign > 0: that share of the
    cells is closed AFTER the route was made, so that paths run over SOLID cells (forced steps)."""
    rng = np.random.default_rng([seed, na, nb, int(density * 100), n_paths, max_look])
    n = na * nb
    blocked = np.where(rng.random((na, nb)) < density, rng.choice(np.array([1, 2, 255], np.uint8), (na, nb)), 0).astype(np.uint8)
    free = np.flatnonzero(blocked.ravel() == 0)
    goal = int(free[rng.integers(0, len(free))]) if len(free) else 0
    starts = rng.integers(0, n, n_paths).astype(np.uint32)
    max_path = max_path or na + nb + 64
    r = (router or R.route_np)(blocked, None, R.params(blocked, max_path=max_path), np.array([goal], np.uint32), starts)
    if foreign:
        blocked = np.where(rng.random((na, nb)) < foreign, 1, blocked).astype(np.uint8)
    dist2 = dist2_brute(blocked) if with_dist2 else None
    return Case(blocked, dist2, r.path, r.path_len, r.path_status, Params(na, nb, max_path, max_look, min_dist2, max_way, cell_size))


def serpentine_case(max_look=8, max_way=64):
    """64 x 64: walls on every fourth row with a gap at alternating ends; the route from one corner to the other is a serpentine of
    about 700 cells."""
    na = nb = 64
    blocked = np.zeros((na, nb), np.uint8)
    for t, ia in enumerate(range(3, na - 1, 6)):
        blocked[ia, :] = 1
        blocked[ia, (nb - 3) if t % 2 == 0 else 0:nb if t % 2 == 0 else 3] = 0
    r = R.route_np(blocked, None, R.params(blocked, max_path=1024), np.array([na * nb - 1], np.uint32), np.array([0], np.uint32))
    return Case(blocked, None, r.path, r.path_len, r.path_status, Params(na, nb, 1024, max_look, 0, max_way, 0.5))


def list_case(na, nb, lists, max_look, blocked=None, dist2=None, status=None, stride=None, min_dist2=0, max_way=16, cell_size=1.0, path_len=None):
    """Paths given as lists of cells."""
    stride = stride or max(max(len(x) for x in lists), 1)
    path = np.full((len(lists), stride), NONE, np.uint32)
    for p, x in enumerate(lists):
        path[p, :min(len(x), stride)] = x[:stride]
    plen = np.array([len(x) for x in lists] if path_len is None else path_len, np.uint32)
    blocked = np.zeros((na, nb), np.uint8) if blocked is None else blocked
    return Case(blocked, dist2, path, plen, None if status is None else np.array(status, np.uint8), Params(na, nb, stride, max_look, min_dist2, max_way, cell_size))


def misreading_cases():
    """The committed inputs on which every misreading differs from the reference (tests/test_grid_waypoints.py asserts it on the
    restatement alone): route-made paths on 17 x 33 at density 0.18 and max_look 8; the same with a dist2 and min_dist2 = 2; paths over
    cells closed after the route was made (forced steps, SOLID ends); a small max_way; a U-turn on open ground whose end is nearer in
    cells than in path entries."""
    u_turn = [1 * 9 + b for b in range(1, 7)] + [2 * 9 + 6] + [3 * 9 + b for b in range(6, 0, -1)]  # out, one down, and back
    return {"route": route_case(17, 33, 0.18, 48, 8, seed=3),
            "detour": list_case(9, 9, [u_turn], 4),
            "dist2": route_case(17, 33, 0.10, 48, 8, seed=5, with_dist2=True, min_dist2=2),
            "foreign": route_case(17, 33, 0.10, 48, 8, seed=9, foreign=0.08),
            "short_way": route_case(17, 33, 0.18, 48, 3, seed=3, max_way=3)}
