"""The voxel map grid's contract (include/svo.h, "Voxel map grid") restated twice, by two routes that share no code, both
applied to a voxel_ref.Table (anything with keys, ci, sx, sy, sz):

  grid_np   whole arrays in numpy: int64 / uint64 arithmetic, np.maximum.at and np.add.at for the four words of a cell;
  grid_py   voxel by voxel in Python integers, into a dict cell -> [top, bot, nvox, npts].

Both return a Grid: cls, top, bottom, intensity, n_voxels, n_points as (na, nb) arrays and the five counts.  `variant` of grid_np
states one deliberate misreading of the contract each; tests/test_voxel_grid.py shows that every one of them changes a grid.
Also here: the scene "street" with the cells its structures stand in, and the constructed single voxels.
Nothing here is tuned on the library's output.
"""
import math
from collections import namedtuple

import numpy as np

import voxel_ref as V

Params = namedtuple("Params", "up_axis up_sign origin_a origin_b cell_voxels na nb up_lo up_hi obstacle_step min_count")
Grid = namedtuple("Grid", "cls top bottom intensity n_voxels n_points counts")
UNKNOWN, LEVEL, OBSTACLE = 0, 1, 2
VARIANTS = ("no_band", "no_sign", "trunc_cell", "key_height", "count_gt", "swap_ab", "mean_intensity", "span_ge")
M64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------ route (a): numpy
def grid_np(table, prm, voxel_size, variant=None):
    vs = np.float64(np.float32(voxel_size))
    with np.errstate(all="ignore"):
        ka0 = int(np.clip(np.floor(np.float64(prm.origin_a) / vs), -2.0 ** 21, 2.0 ** 21))
        kb0 = int(np.clip(np.floor(np.float64(prm.origin_b) / vs), -2.0 ** 21, 2.0 ** 21))
        hlo = int(np.clip(np.floor(np.float64(prm.up_lo) / vs * 65536.0), -2.0 ** 38, 2.0 ** 38))
        hhi = int(np.clip(np.floor(np.float64(prm.up_hi) / vs * 65536.0), -2.0 ** 38, 2.0 ** 38))
        step = int(np.clip(np.floor(np.float64(prm.obstacle_step) / vs * 65536.0), 0.0, 2.0 ** 38))
    keys, ci = np.asarray(table.keys, np.uint64), np.asarray(table.ci, np.uint64)
    sums = [np.asarray(s, np.uint64) for s in (table.sx, table.sy, table.sz)]
    count = ci >> np.uint64(40)
    isum = ci & np.uint64((1 << 40) - 1)
    ok = keys != np.uint64(V.EMPTY)
    ok &= (count > np.uint64(prm.min_count)) if variant == "count_gt" else (count >= np.uint64(prm.min_count))
    n_qual = int(ok.sum())
    keys, count, isum, sums = keys[ok], count[ok], isum[ok], [s[ok] for s in sums]
    idx = [((keys >> np.uint64(21 * r)) & np.uint64(0x1FFFFF)).astype(np.int64) - (1 << 20) for r in range(3)]
    up = prm.up_axis
    a, b = ((up + 2) % 3, (up + 1) % 3) if variant == "swap_ab" else ((up + 1) % 3, (up + 2) % 3)
    g = idx[up] * 65536
    if variant != "key_height":
        g = g + (sums[up] // count).astype(np.int64)
    hgt = g if variant == "no_sign" else prm.up_sign * g
    band = np.ones(len(hgt), bool) if variant == "no_band" else (hgt >= hlo) & (hgt <= hhi)
    n_band = int(band.sum())
    da, db = idx[a] - ka0, idx[b] - kb0
    if variant == "trunc_cell":
        ia, ib = np.trunc(da / prm.cell_voxels).astype(np.int64), np.trunc(db / prm.cell_voxels).astype(np.int64)
    else:
        ia, ib = da // prm.cell_voxels, db // prm.cell_voxels  # numpy's // on signed integers is the floor
    inside = band & (ia >= 0) & (ia < prm.na) & (ib >= 0) & (ib < prm.nb)
    n_bin = int(inside.sum())
    cell = (ia * prm.nb + ib)[inside]
    hgt, count, isum = hgt[inside], count[inside], isum[inside]
    n = prm.na * prm.nb
    top, bot, nvox, npts = (np.zeros(n, np.uint64) for _ in range(4))
    word = ((hgt + (1 << 37)).astype(np.uint64) << np.uint64(8)) | (isum // count)
    np.maximum.at(top, cell, word)
    np.maximum.at(bot, cell, ((1 << 37) - hgt).astype(np.uint64))
    np.add.at(nvox, cell, np.uint64(1))
    np.add.at(npts, cell, count)
    # resolve
    some = nvox > 0
    htop = (top >> np.uint64(8)).astype(np.int64) - (1 << 37)
    hbot = (1 << 37) - bot.astype(np.int64)
    span = htop - hbot
    cls = np.where(some, np.where((span >= step) if variant == "span_ge" else (span > step), OBSTACLE, LEVEL), UNKNOWN).astype(np.uint8)
    t = np.where(some, (htop.astype(np.float64) / 65536.0 * vs).astype(np.float32), np.float32(-np.inf)).astype(np.float32)
    bt = np.where(some, (hbot.astype(np.float64) / 65536.0 * vs).astype(np.float32), np.float32(np.inf)).astype(np.float32)
    inten = (top & np.uint64(255)).astype(np.uint8)
    if variant == "mean_intensity":
        all_i = np.zeros(n, np.uint64)
        np.add.at(all_i, cell, isum)
        inten = np.where(some, all_i // np.maximum(npts, np.uint64(1)), 0).astype(np.uint8)
    shape = (prm.na, prm.nb)
    counts = (n_qual, n_band, n_bin, int(some.sum()), int((cls == OBSTACLE).sum()))
    return Grid(cls.reshape(shape), t.reshape(shape), bt.reshape(shape), inten.reshape(shape), nvox.astype(np.uint32).reshape(shape),
                npts.reshape(shape), counts)


# ------------------------------------------------------------------------------------------------ route (b): Python
def _floor_clamped(x, lo, hi):
    """clamp(floor(x), lo, hi) for a float x that may be infinite."""
    if x <= lo:
        return int(lo)
    if x >= hi:
        return int(hi)
    return math.floor(x)


def grid_py(table, prm, voxel_size):
    vs = float(np.float32(voxel_size))
    far, high = float(1 << 21), float(1 << 38)
    ka0, kb0 = _floor_clamped(prm.origin_a / vs, -far, far), _floor_clamped(prm.origin_b / vs, -far, far)
    hlo, hhi = _floor_clamped(prm.up_lo / vs * 65536.0, -high, high), _floor_clamped(prm.up_hi / vs * 65536.0, -high, high)
    step = _floor_clamped(prm.obstacle_step / vs * 65536.0, 0.0, high)
    ax_up, ax_a, ax_b = prm.up_axis, (prm.up_axis + 1) % 3, (prm.up_axis + 2) % 3
    cells = {}
    n_qual = n_band = n_bin = 0
    for key, ci, sx, sy, sz in zip(*(np.asarray(v).tolist() for v in (table.keys, table.ci, table.sx, table.sy, table.sz))):
        count = ci >> 40
        if key == V.EMPTY or count < prm.min_count:
            continue
        n_qual += 1
        k = [((key >> (21 * r)) & 0x1FFFFF) - (1 << 20) for r in range(3)]
        g = k[ax_up] * 65536 + (sx, sy, sz)[ax_up] // count
        hgt = g if prm.up_sign > 0 else -g
        if not (hlo <= hgt <= hhi):
            continue
        n_band += 1
        ia, ib = (k[ax_a] - ka0) // prm.cell_voxels, (k[ax_b] - kb0) // prm.cell_voxels  # Python's // is the floor
        if not (0 <= ia < prm.na and 0 <= ib < prm.nb):
            continue
        n_bin += 1
        c = cells.setdefault(ia * prm.nb + ib, [0, 0, 0, 0])
        c[0] = max(c[0], (((hgt + (1 << 37)) << 8) & M64) | ((ci & ((1 << 40) - 1)) // count))
        c[1] = max(c[1], ((1 << 37) - hgt) & M64)
        c[2] += 1
        c[3] += count
    grid_py.last = cells
    shape = (prm.na, prm.nb)
    cls, inten = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    top, bottom = np.full(shape, -np.inf, np.float32), np.full(shape, np.inf, np.float32)
    nvox, npts = np.zeros(shape, np.uint32), np.zeros(shape, np.uint64)
    n_obstacle = 0
    for cell, (t, b, nv, npt) in cells.items():
        at = divmod(cell, prm.nb)
        htop, hbot = (t >> 8) - (1 << 37), (1 << 37) - b
        cls[at] = OBSTACLE if htop - hbot > step else LEVEL
        n_obstacle += int(cls[at] == OBSTACLE)
        top[at], bottom[at] = np.float32(float(htop) / 65536.0 * vs), np.float32(float(hbot) / 65536.0 * vs)
        inten[at], nvox[at], npts[at] = t & 255, nv, npt
    return Grid(cls, top, bottom, inten, nvox, npts, (n_qual, n_band, n_bin, len(cells), n_obstacle))


def same(a, b):
    """== on everything; top and bottom as bit patterns."""
    return all(np.array_equal(getattr(a, n), getattr(b, n)) for n in ("cls", "intensity", "n_voxels", "n_points")) and \
        np.array_equal(a.top.view(np.uint32), b.top.view(np.uint32)) and np.array_equal(a.bottom.view(np.uint32), b.bottom.view(np.uint32)) and \
        tuple(a.counts) == tuple(b.counts)


def cell_of(prm, voxel_size, a, b):
    """Item 4 for a position in map units: (inside, ia, ib)."""
    vs = float(np.float32(voxel_size))
    far = float(1 << 21)
    ia = (_floor_clamped(a / vs, -far, far) - _floor_clamped(prm.origin_a / vs, -far, far)) // prm.cell_voxels
    ib = (_floor_clamped(b / vs, -far, far) - _floor_clamped(prm.origin_b / vs, -far, far)) // prm.cell_voxels
    return 0 <= ia < prm.na and 0 <= ib < prm.nb, ia, ib


# ------------------------------------------------------------------------------------------------ the scene "street"
STREET_SIZES = ((0.05, 16, 10), (0.1, 15, 5), (0.25, 13, 2))  # voxel size, table log2, cell_voxels of a 0.5 m cell


def street_params(cell_voxels, min_count=1):
    """The camera convention (y down: up_axis 1, up_sign -1; a = z forward, b = x right), 32 x 13 cells of 0.5 m from z = 0 and
    x = -3.2, the band -2.5 .. 2.0, step 0.3."""
    return Params(1, -1, 0.0, -3.2, cell_voxels, 32, 13, -2.5, 2.0, 0.3, min_count)


def street(seed=7):
    """World-frame records (identity transform, y down), 0.06 m apart, every lattice a few millimetres off the voxel faces:
      road      x in [-4, 4), z in [2, 14), y = 1.5 + 0.02 z +- 0.01, raised by 0.12 where x > 2.5 (the kerb);
      box       0.8 x 0.8 x 1.0 at x in [-1, -0.2), z in [5, 5.8): its front and top faces;
      wall      3 m high at z = 12 + 0.03 x;
      overhang  y = -2.5 over x in [-1, 1), z in [8, 9): above the band;
      post      one point per 0.1 m at x = 1.03, z = 7.03, y from 0.5 to 1.6."""
    rng = np.random.default_rng(seed)
    step, ox, oz = 0.06, 0.013, 0.017
    parts = []

    def add(x, y, z):
        x, y, z = np.broadcast_arrays(x, y, z)
        parts.append((x.ravel(), y.ravel(), z.ravel()))

    xs, zs = np.arange(-4.0 + ox, 4.0, step), np.arange(2.0 + oz, 14.0, step)
    X, Z = np.meshgrid(xs, zs)
    add(X, 1.5 + 0.02 * Z + rng.uniform(-0.01, 0.01, X.shape) - np.where(X > 2.5, 0.12, 0.0), Z)
    bx, bz, by = np.arange(-1.0 + ox, -0.2, step), np.arange(5.0 + oz, 5.8, step), np.arange(0.6 + 0.011, 1.6, step)
    X, Y = np.meshgrid(bx, by)
    add(X, Y, 5.0 + oz)  # the front face
    X, Z = np.meshgrid(bx, bz)
    add(X, 0.6 + 0.011, Z)  # the top face
    X, Y = np.meshgrid(xs, np.arange(-1.26 + 0.011, 1.74, step))
    add(X, Y, 12.0 + 0.03 * X)
    X, Z = np.meshgrid(np.arange(-1.0 + ox, 1.0, step), np.arange(8.0 + oz, 9.0, step))
    add(X, -2.5, Z)
    py = np.arange(0.5, 1.6 + 1e-9, 0.1)
    add(1.03, py, 7.03)
    x, y, z = (np.concatenate([p[i] for p in parts]).astype(np.float32) for i in range(3))
    tag = np.arange(len(x), dtype=np.uint32) & np.uint32(0xFFFFFF) | (rng.integers(0, 256, len(x)).astype(np.uint32) << np.uint32(24))
    return V.records(x, y, z, tag)


def street_cells(prm, voxel_size):
    """name -> the set of cells (ia, ib) a structure of the scene stands in, from positions well inside it, by the grid's rule."""
    at = lambda z, x: cell_of(prm, voxel_size, z, x)[1:]
    return {
        "kerb": {at(z, 2.5) for z in np.arange(2.25, 11.5, 0.5)},
        "under_overhang": {at(z, x) for z in (8.25, 8.75) for x in (-0.9, -0.4, 0.1, 0.6)},
        "box": {at(z, x) for z in (5.3, 5.7) for x in (-0.9, -0.45)},
        "wall": {at(12.0 + 0.03 * x, x) for x in np.arange(-2.95, 3.3, 0.5)},
        "post": {at(7.03, 1.03)},
    }


# ------------------------------------------------------------------------------------------------ constructed voxels
CONSTRUCTED_VS = 0.25  # exact in f32: a coordinate p gives q = 4 p exactly


def constructed_params(**kw):
    """Voxel size 0.25, the camera convention, 3 x 2 cells of 2 voxels from z = 0.25 (ka0 = 1) and x = -0.5 (kb0 = -2): cells cover
    k_z in 1..6 and k_x in -2..1.  The band -1 .. 2 is hlo = -262144, hhi = 524288; obstacle_step 0.5 is step = 131072."""
    return Params(1, -1, 0.25, -0.5, 2, 3, 2, -1.0, 2.0, 0.5, 1)._replace(**kw)


def _at(kz, kx, hgt, inten=0x40, n=1):
    """n records in the voxel with the key indices (k_x, ., k_z) whose height along up = -y is exactly hgt 65536ths of a voxel."""
    y = -float(hgt) / 65536.0 * CONSTRUCTED_VS
    assert float(np.float32(y)) == y
    return V.records(np.float32([kx * 0.25 + 0.1] * n), np.float32([y] * n), np.float32([kz * 0.25 + 0.1] * n), np.uint32([inten << 24] * n))


def constructed():
    """name -> (records, Params, facts): facts is a dict cell (ia, ib) -> (cls, htop, hbot, intensity, n_voxels, n_points) of every
    occupied cell, in 65536ths of a voxel, plus the key "counts" -> (n_qualifying, n_in_band, n_binned)."""
    P = constructed_params()
    hlo, hhi, step = -262144, 524288, 131072
    cat = np.concatenate
    out = {
        # a span of exactly step is LEVEL, one 65536th more is an OBSTACLE
        "span_step": (cat([_at(1, -2, 0), _at(2, -2, step), _at(1, 0, 0), _at(2, 0, step + 1)]), P,
                      {(0, 0): (LEVEL, step, 0, 0x40, 2, 2), (0, 1): (OBSTACLE, step + 1, 0, 0x40, 2, 2), "counts": (4, 4, 4)}),
        # the band's ends are inside
        "band_ends": (cat([_at(3, -2, hlo - 1), _at(4, -2, hlo), _at(3, 0, hhi), _at(4, 0, hhi + 1)]), P,
                      {(1, 0): (LEVEL, hlo, hlo, 0x40, 1, 1), (1, 1): (LEVEL, hhi, hhi, 0x40, 1, 1), "counts": (4, 2, 2)}),
        # k_a - ka0 at -1, 0, na cell_voxels - 1, na cell_voxels: the first and the last are outside
        "edges_a": (cat([_at(0, -2, 5), _at(1, -2, 6), _at(6, -2, 7), _at(7, -2, 8)]), P,
                    {(0, 0): (LEVEL, 6, 6, 0x40, 1, 1), (2, 0): (LEVEL, 7, 7, 0x40, 1, 1), "counts": (4, 4, 2)}),
        "edges_b": (cat([_at(3, -3, 5), _at(3, -2, 6), _at(3, 1, 7), _at(3, 2, 8)]), P,
                    {(1, 0): (LEVEL, 6, 6, 0x40, 1, 1), (1, 1): (LEVEL, 7, 7, 0x40, 1, 1), "counts": (4, 4, 2)}),
        # equal heights: the larger mean intensity wins the cell, in either order
        "equal_height": (cat([_at(1, -2, 100, 0x20), _at(2, -2, 100, 0x90)]), P, {(0, 0): (LEVEL, 100, 100, 0x90, 2, 2), "counts": (2, 2, 2)}),
        "equal_height_2": (cat([_at(1, -2, 100, 0x90), _at(2, -2, 100, 0x20)]), P, {(0, 0): (LEVEL, 100, 100, 0x90, 2, 2), "counts": (2, 2, 2)}),
        # 300 identical records: n_points, and both divisions at a count of 300
        "many_points": (_at(5, 1, -40000, 0x77, 300), P, {(2, 1): (LEVEL, -40000, -40000, 0x77, 1, 300), "counts": (1, 1, 1)}),
        # s = 600 * 40000 - 1: s / c = 39999.998..., which f32 rounds UP to 40000.0 (its spacing there is 2^-8, and s itself is
        # past 2^24); the floor is 39999.  (No s < 2^40 brings a correctly rounded f64 quotient across an integer: s / c is at least
        # 1 / c away from one and f64's spacing at s / c is below 2^-12 / c.  An f64 product with a reciprocal can cross; f32 does.)
        "quotient_rounds_up": (cat([_at(5, 1, -40000, 0x10, 599), _at(5, 1, -39999, 0x0F)]), P,
                               {(2, 1): (LEVEL, -39999, -39999, 0x0F, 1, 600), "counts": (1, 1, 1)}),
        # min_count: a count of exactly min_count qualifies
        "min_count": (cat([_at(1, -2, 3, n=3), _at(2, -2, 9, n=2)]), constructed_params(min_count=3),
                      {(0, 0): (LEVEL, 3, 3, 0x40, 1, 3), "counts": (1, 1, 1)}),
    }
    return out
