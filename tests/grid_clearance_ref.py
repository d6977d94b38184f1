"""The ground plan clearance's contract (include/svo.h, "Ground plan clearance") restated twice, by two routes that share
no code, both applied to an (na, nb) uint8 class grid:

  clearance_np   whole arrays in numpy: for every row of cells the squared distances to ALL sources of the rows within max_dist
                 (a source in a row farther away is farther than max_dist, so rule 2 gives NONE for it anyway), source blocks in
                 chunks, the tie broken by the min over the indices masked to the attaining sources;
  clearance_py   cell by cell in Python integers: over the list of sources, or, where that is the longer way, over the disc's
                 offsets by growing squared distance until one ring holds a source.

Neither is the separable search of the kernels.  Both return a Clearance: dist2, nearest (uint32), clearance (float32), blocked
(uint8) as (na, nb) arrays and the four counts.  `variant` of clearance_np states one deliberate misreading of the contract each;
tests/test_grid_clearance.py shows that every one of them changes a result.  Also here: the seeded random grids and the constructed
ones with the facts they were built for.  Nothing here is tuned on the library's output.
"""
import functools
from collections import namedtuple

import numpy as np

Params = namedtuple("Params", "na nb source_mask max_dist cell_size inflate_radius")
Clearance = namedtuple("Clearance", "dist2 nearest clearance blocked counts")
NONE = 0xFFFFFFFF
VARIANTS = ("tie_larger", "lt_max", "square", "chessboard", "manhattan", "row_left_only", "none_for_sources", "wrap32")
_BIG = np.int32(2 ** 31 - 1)


def params(cls, max_dist, source_mask=1 << 2, cell_size=0.5, inflate_radius=0.0):
    return Params(cls.shape[0], cls.shape[1], source_mask, max_dist, cell_size, inflate_radius)


def r2_of(prm):
    """Rule 5's R2: floor((inflate_radius / cell_size)^2) in f64, clamped to max_dist^2."""
    with np.errstate(all="ignore"):
        rc = np.float64(prm.inflate_radius) / np.float64(prm.cell_size)
        q = rc * rc
    cap = prm.max_dist * prm.max_dist
    return cap if q >= cap else int(np.floor(q))


def _finish(cls, prm, d2, near, src, variant=None):
    """Rules 4 to 6 from dist2, nearest and the source mask."""
    d2, near = d2.astype(np.uint32), near.astype(np.uint32)
    if variant == "none_for_sources":
        d2[src], near[src] = NONE, NONE
    none = d2 == NONE
    with np.errstate(all="ignore"):
        clearance = (np.sqrt(d2.astype(np.float64)) * np.float64(prm.cell_size)).astype(np.float32)
    clearance[none] = np.inf
    blocked = np.where(src, 2, np.where(~none & (d2 <= r2_of(prm)), 1, 0)).astype(np.uint8)
    counts = (int(src.sum()), int((~src & ~none).sum()), int(none.sum()), int((blocked == 1).sum()))
    return Clearance(d2, near, clearance, blocked, counts)


# ------------------------------------------------------------------------------------------------ route (a): numpy
def sources_np(cls, mask, variant=None):
    c = np.asarray(cls, np.uint8).astype(np.int64)
    if variant == "wrap32":
        return ((np.int64(mask) >> (c & 31)) & 1).astype(bool)
    return (c < 32) & (((np.int64(mask) >> np.minimum(c, 31)) & 1) == 1)


def clearance_np(cls, prm, variant=None, chunk=8192):
    na, nb, md = prm.na, prm.nb, prm.max_dist
    assert cls.shape == (na, nb) and cls.dtype == np.uint8
    src = sources_np(cls, prm.source_mask, variant)
    sidx = np.flatnonzero(src.ravel()).astype(np.int32)  # ascending
    sa, sb = sidx // nb, sidx % nb
    ib = np.arange(nb, dtype=np.int32)
    d2 = np.full((na, nb), NONE, np.int64)
    near = np.full((na, nb), NONE, np.int64)
    cap = md * md
    for ia in range(na):
        lo, hi = np.searchsorted(sa, ia - md, "left"), np.searchsorted(sa, ia + md, "right")
        best = np.full(nb, _BIG, np.int32)
        at = np.full(nb, -1 if variant == "tie_larger" else _BIG, np.int32)
        for c0 in range(lo, hi, chunk):
            a, b, idx = sa[c0:min(c0 + chunk, hi)], sb[c0:min(c0 + chunk, hi)], sidx[c0:min(c0 + chunk, hi)]
            da, db = np.abs(ia - a)[None, :], np.abs(ib[:, None] - b[None, :])
            if variant == "chessboard":
                d = np.maximum(da, db) ** 2
            elif variant == "manhattan":
                d = (da + db) ** 2
            else:
                d = da * da + db * db
            if variant == "square":
                d = np.where(db <= md, d, _BIG)  # the rows are within max_dist already
            if variant == "row_left_only":
                d = np.where(b[None, :] <= ib[:, None], d, _BIG)
            m = d.min(axis=1)
            if variant == "tie_larger":
                j = np.where(d == m[:, None], idx[None, :], -1).max(axis=1)
                take = (m < best) | ((m == best) & (j > at))
            else:
                j = np.where(d == m[:, None], idx[None, :], _BIG).min(axis=1)
                take = (m < best) | ((m == best) & (j < at))
            best, at = np.where(take, m, best), np.where(take, j, at)
        if variant == "square":
            ok = best < _BIG
        elif variant == "lt_max":
            ok = best < cap
        else:
            ok = best <= cap
        d2[ia], near[ia] = np.where(ok, best, NONE), np.where(ok, at, NONE)
    return _finish(cls, prm, d2, near, src, variant)


# ------------------------------------------------------------------------------------------------ route (b): Python integers
@functools.lru_cache(maxsize=None)
def _rings(md):
    """The disc's offsets grouped by squared distance, ascending."""
    rings = {}
    for di in range(-md, md + 1):
        for dj in range(-md, md + 1):
            if di * di + dj * dj <= md * md:
                rings.setdefault(di * di + dj * dj, []).append((di, dj))
    return sorted(rings.items())


def clearance_py(cls, prm, cells=None):
    """cells: the flat indices to do (None: all); the others come back as NONE / not counted, for grids too large to walk whole."""
    na, nb, md, mask = prm.na, prm.nb, prm.max_dist, prm.source_mask
    rows = [[int(v) for v in row] for row in cls]
    is_src = [[v < 32 and (mask >> v) & 1 == 1 for v in row] for row in rows]
    srcs = [(ja, jb) for ja in range(na) for jb in range(nb) if is_src[ja][jb]]
    rings = _rings(md)
    # a ring search ends after about cells / sources offsets, and after the whole disc at the latest
    by_list = len(srcs) <= min(sum(len(r) for _, r in rings), na * nb // max(len(srcs), 1))
    try:
        rc = float(prm.inflate_radius) / float(prm.cell_size)
    except OverflowError:  # Python raises where IEEE division gives +infinity
        rc = float("inf")
    r2 = md * md if rc * rc >= md * md else int(rc * rc // 1)
    d2 = np.full((na, nb), NONE, np.uint32)
    near = np.full((na, nb), NONE, np.uint32)
    clearance = np.full((na, nb), np.inf, np.float32)
    blocked = np.zeros((na, nb), np.uint8)
    counts = [0, 0, 0, 0]
    for cell in (range(na * nb) if cells is None else cells):
        ia, ib = divmod(cell, nb)
        best = None
        if by_list:
            for ja, jb in srcs:  # ascending index: a later source must be strictly nearer
                d = (ia - ja) * (ia - ja) + (ib - jb) * (ib - jb)
                if best is None or d < best[0]:
                    best = (d, ja * nb + jb)
            if best is not None and best[0] > md * md:
                best = None
        else:
            for d, ring in rings:
                hit = [(ia + di) * nb + ib + dj for di, dj in ring if 0 <= ia + di < na and 0 <= ib + dj < nb and is_src[ia + di][ib + dj]]
                if hit:
                    best = (d, min(hit))
                    break
        if best is None:
            counts[2] += 1
            continue
        d2[ia, ib], near[ia, ib] = best
        clearance[ia, ib] = np.float32(np.sqrt(np.float64(best[0])) * np.float64(prm.cell_size))
        if best[0] == 0:
            blocked[ia, ib] = 2
            counts[0] += 1
        else:
            counts[1] += 1
            if best[0] <= r2:
                blocked[ia, ib] = 1
                counts[3] += 1
    return Clearance(d2, near, clearance, blocked, tuple(counts))


def same(a, b, cells=None):
    pick = (lambda x: x) if cells is None else (lambda x: x.ravel()[list(cells)])
    return (all(np.array_equal(pick(getattr(a, k)), pick(getattr(b, k))) for k in ("dist2", "nearest", "blocked"))
            and np.array_equal(pick(a.clearance).view(np.uint32), pick(b.clearance).view(np.uint32)) and (cells is not None or a.counts == b.counts))


# ------------------------------------------------------------------------------------------------ the grids
SIZES = ((1, 1), (1, 257), (257, 1), (2, 2), (63, 65), (64, 64), (65, 63), (256, 256), (130, 300))
MAX_DISTS = (1, 5, 64)
DENSITIES = (0.002, 0.05, 0.5)


@functools.lru_cache(maxsize=None)
def random_grid(na, nb, density, seed=0x5EED0C1E):
    """Classes 0 / 1 / 2 (2 with probability `density`) and, rarely, values that are never sources (40, 255)."""
    rng = np.random.default_rng([seed, na, nb, int(density * 1000)])
    cls = rng.integers(0, 2, (na, nb)).astype(np.uint8)
    cls[rng.random((na, nb)) < 0.01] = 40
    cls[rng.random((na, nb)) < 0.01] = 255
    cls[rng.random((na, nb)) < density] = 2
    cls.setflags(write=False)
    return cls


def _grid(na, nb, at, fill=1):
    cls = np.full((na, nb), fill, np.uint8)
    for ia, ib in at:
        cls[ia, ib] = 2
    return cls


def constructed():
    """name -> (cls, Params, facts): facts maps (ia, ib) -> (dist2, nearest) that the case was built to give, "counts" -> the four."""
    out = {}
    c = _grid(9, 11, [])
    out["no_source"] = (c, params(c, 64), {"counts": (0, 0, 99, 0), (0, 0): (NONE, NONE), (8, 10): (NONE, NONE)})
    c = np.full((7, 9), 2, np.uint8)
    out["all_sources"] = (c, params(c, 5, inflate_radius=3.0), {"counts": (63, 0, 0, 0), (0, 0): (0, 0), (6, 8): (0, 62), (3, 4): (0, 31)})
    c = _grid(20, 23, [(0, 0), (0, 22), (19, 0), (19, 22)])
    out["corners"] = (c, params(c, 64), {"counts": (4, 456, 0, 0), (9, 11): (9 * 9 + 11 * 11, 0), (10, 11): (9 * 9 + 11 * 11, 19 * 23),
                                         (9, 12): (9 * 9 + 10 * 10, 22), (10, 12): (9 * 9 + 10 * 10, 19 * 23 + 22), (0, 11): (121, 0)})
    c = _grid(13, 13, [(6, 6)])  # 81 cells of the disc of radius 5 but the source; the window's corners are NONE
    out["disc"] = (c, params(c, 5), {"counts": (1, 80, 88, 0), (9, 10): (25, 84), (10, 10): (NONE, NONE), (6, 11): (25, 84), (6, 12): (NONE, NONE),
                                     (1, 6): (25, 84), (0, 6): (NONE, NONE)})
    c = _grid(5, 5, [(1, 2), (2, 1), (2, 3), (3, 2)])
    out["four_way_tie"] = (c, params(c, 5), {"counts": (4, 21, 0, 0), (2, 2): (1, 7), (1, 1): (1, 7), (3, 3): (1, 13), (3, 1): (1, 11)})
    c = _grid(7, 7, [(1, 3), (4, 6)])  # (4, 3): its own row's source at g = 3 is met first, the one three rows up has the smaller index
    out["earlier_row_tie"] = (c, params(c, 64), {"counts": (2, 47, 0, 0), (4, 3): (9, 10), (5, 3): (10, 4 * 7 + 6), (4, 4): (4, 4 * 7 + 6)})
    c = _grid(3, 9, [(1, 2), (1, 6)])
    out["row_tie"] = (c, params(c, 64), {"counts": (2, 25, 0, 0), (1, 4): (4, 11), (0, 4): (5, 11), (2, 4): (5, 11), (1, 5): (1, 15)})
    c = _grid(6, 12, [(2, 8), (4, 3)])  # (2, 2): the row's own source is 6 away, beyond max_dist 3; (4, 3) is at 4 + 1
    out["through_another_row"] = (c, params(c, 3), {"counts": (2, 47, 23, 0), (2, 2): (5, 51), (2, 4): (5, 51), (2, 5): (8, 51), (2, 6): (4, 32), (2, 3): (4, 51),
                                                    (0, 3): (NONE, NONE)})
    return out


def all_values():
    """Every byte value once, 16 x 16, and the masks that pick one class, two, the last bit and every bit."""
    cls = np.arange(256, dtype=np.uint8).reshape(16, 16)
    return cls, (1 << 2, 1 << 0 | 1 << 2, 1 << 31, 0xFFFFFFFF)
