"""The ground plan surface's contract (include/svo.h, "Ground plan surface") restated twice, by two routes that share no
code, both applied to an (na, nb) uint8 class grid and its float32 tops:

  surface_py   cell by cell in plain Python: floats through struct (f32 <-> f64) and math, the footprint as a list of offsets, the
               rules in the order the contract states them; it can be asked for a list of cells only;
  surface_np   whole arrays in numpy: the grid padded by 15 cells of "nothing there", the step by four shifted views, hi, lo and the
               support by one pass per footprint offset.

Neither stages tiles or walks rows by a half-width table, as the kernel does.  Both return a Surface: cls_out (uint8), step and
relief (float32), support (uint16) as (na, nb) arrays and the six counts.  `variant` of surface_np states one deliberate misreading
of the contract each; tests/test_grid_surface.py shows that every one of them changes a stated case by a stated count.  Also here:
the seeded random cases and the constructed grids with the facts they were built for.  Nothing here is tuned on the library's output.

One constructed pair differs from the issue's wording on purpose and is kept BESIDE the pair it names: 16777216.0f - 1.0f is
16777215, which f32 holds exactly, so no threshold tells the f32 subtraction from the f64 one there ("big_exact" asserts just that);
16777216.0f - (-1.0f) is 16777217 in f64 and 16777216 in f32, and "big_f32_wrong" puts max_step between the two.
"""
import math
import struct
from collections import namedtuple

import numpy as np

Params = namedtuple("Params", "na nb ground_mask cell_size max_step footprint_radius max_relief min_support_256")
Surface = namedtuple("Surface", "cls_out step relief support counts")
STEP, ROUGH, UNSUPPORTED = 3, 4, 5
SOURCES = 1 << 2 | 1 << 3 | 1 << 4 | 1 << 5
COUNTS = ("n_ground", "n_step", "n_rough", "n_unsupported", "n_nonfinite", "n_kept")
VARIANTS = ("step8", "step_ge", "relief_ge", "square", "nonground_heights", "outside_support", "rough_first", "f32_sub", "nonfinite_through")
INF = float("inf")
PAD = 15
F03 = float(np.float32(0.3))  # (double)0.3f


def params(cls, r2=2, ground_mask=1 << 1, cell_size=0.5, max_step=0.3, max_relief=0.6, min_support_256=0):
    """A parameter set whose footprint has exactly this r2: rc = sqrt(r2) nudged up so that floor(rc * rc) is r2 at this cell size."""
    radius = radius_for(r2, cell_size)
    return Params(cls.shape[0], cls.shape[1], ground_mask, cell_size, max_step, radius, max_relief, min_support_256)


def radius_for(r2, cell_size=0.5):
    radius = math.sqrt(r2) * cell_size
    while r2_of_radius(radius, cell_size) < r2:
        radius = math.nextafter(radius, INF)
    assert r2_of_radius(radius, cell_size) == r2
    return radius


def r2_of_radius(radius, cell_size):
    rc = radius / cell_size
    q = rc * rc
    assert q < 226.0
    return int(math.floor(q))


def r2_of(prm):
    return r2_of_radius(prm.footprint_radius, prm.cell_size)


def footprint(r2, square=False):
    rw = math.isqrt(r2)
    return [(da, db) for da in range(-rw, rw + 1) for db in range(-rw, rw + 1) if square or da * da + db * db <= r2]


def cells_of(r2):
    """D(r2)."""
    return len(footprint(r2))


def half_widths(r2):
    rw = math.isqrt(r2)
    return [math.isqrt(r2 - da * da) for da in range(-rw, rw + 1)]


# ------------------------------------------------------------------------------------------------ route (a): Python, cell by cell
def _to_f32(x):
    """The f64 x rounded to f32, as the f64 that holds it."""
    try:
        return struct.unpack("<f", struct.pack("<f", x))[0]
    except OverflowError:
        return math.copysign(INF, x)


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def surface_py(cls, top, prm, cells=None):
    """Rules 1 to 6 for the listed cells (all of them when None).  Returns {(ia, ib): (cls_out, step bits, relief bits, support,
    what)} with what one of "ground:step", "ground:rough", "ground:unsupported", "ground:kept", "nonfinite", "other"."""
    na, nb = prm.na, prm.nb
    raw = [[struct.unpack("<f", struct.pack("<f", float(top[ia, ib])))[0] for ib in range(nb)] for ia in range(na)]
    c = [[int(cls[ia, ib]) for ib in range(nb)] for ia in range(na)]
    r2 = r2_of(prm)
    fp = footprint(r2)
    D = len(fp)

    def in_mask(ia, ib):
        return c[ia][ib] < 32 and (prm.ground_mask >> c[ia][ib]) & 1 == 1

    def ground(ia, ib):
        return 0 <= ia < na and 0 <= ib < nb and in_mask(ia, ib) and math.isfinite(raw[ia][ib])

    out = {}
    todo = cells if cells is not None else [(ia, ib) for ia in range(na) for ib in range(nb)]
    for ia, ib in todo:
        support = sum(1 for da, db in fp if ground(ia + da, ib + db))
        if not ground(ia, ib):
            if in_mask(ia, ib):
                out[ia, ib] = (UNSUPPORTED, _bits(-1.0), _bits(-1.0), support, "nonfinite")
            else:
                out[ia, ib] = (c[ia][ib], _bits(-1.0), _bits(-1.0), support, "other")
            continue
        t = raw[ia][ib]
        dstep = 0.0
        for da, db in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            if ground(ia + da, ib + db):
                dstep = max(dstep, abs(t - raw[ia + da][ib + db]))
        heights = [raw[ia + da][ib + db] for da, db in fp if ground(ia + da, ib + db)]
        hi, lo = max(heights), min(heights)
        drelief = hi - lo if hi > lo else 0.0
        if dstep > prm.max_step:
            k, what = STEP, "ground:step"
        elif drelief > prm.max_relief:
            k, what = ROUGH, "ground:rough"
        elif support * 256 < prm.min_support_256 * D:
            k, what = UNSUPPORTED, "ground:unsupported"
        else:
            k, what = c[ia][ib], "ground:kept"
        out[ia, ib] = (k, _bits(_to_f32(dstep)), _bits(_to_f32(drelief)), support, what)
    return out


def as_surface(cells, prm):
    """A Surface from surface_py's result over every cell."""
    na, nb = prm.na, prm.nb
    arr = lambda k, t: np.array([[cells[ia, ib][k] for ib in range(nb)] for ia in range(na)], t).reshape(na, nb)
    what = [v[4] for v in cells.values()]
    n = {w: what.count(w) for w in set(what)}
    g = [n.get("ground:" + k, 0) for k in ("step", "rough", "unsupported", "kept")]
    counts = (sum(g), g[0], g[1], g[2], n.get("nonfinite", 0), g[3])
    return Surface(arr(0, np.uint8), arr(1, np.uint32).view(np.float32), arr(2, np.uint32).view(np.float32), arr(3, np.uint16), counts)


# ------------------------------------------------------------------------------------------------ route (b): numpy, whole arrays
def in_mask_np(cls, mask):
    c = np.asarray(cls, np.uint8).astype(np.int64)
    return (c < 32) & (((np.int64(mask) >> np.minimum(c, 31)) & 1) == 1)


def surface_np(cls, top, prm, variant=None, detail=False):
    """detail: also return the three conditions of rule 6 per cell, (a, b, c), False where the cell is not GROUND."""
    na, nb = prm.na, prm.nb
    assert cls.shape == (na, nb) == top.shape and cls.dtype == np.uint8 and top.dtype == np.float32
    assert variant is None or variant in VARIANTS
    r2 = r2_of(prm)
    inm = in_mask_np(cls, prm.ground_mask)
    fin = np.isfinite(top)
    ground = inm & fin
    nonfinite = inm & ~fin
    gives = fin if variant == "nonground_heights" else ground  # whose height is looked at
    gp = np.zeros((na + 2 * PAD, nb + 2 * PAD), bool)
    hp = np.zeros(gp.shape, bool)
    tp = np.zeros(gp.shape, np.float32)
    if variant == "outside_support":
        gp[:] = True
    gp[PAD:PAD + na, PAD:PAD + nb] = ground
    hp[PAD:PAD + na, PAD:PAD + nb] = gives
    tp[PAD:PAD + na, PAD:PAD + nb] = np.where(fin, top, np.float32(0))
    win = lambda a, da, db: a[PAD + da:PAD + da + na, PAD + db:PAD + db + nb]
    t64 = top.astype(np.float64)
    dstep = np.zeros((na, nb), np.float64)
    edges = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if variant == "step8" else [])
    with np.errstate(all="ignore"):
        for da, db in edges:
            if variant == "f32_sub":
                d = np.abs(np.where(fin, top, np.float32(0)) - win(tp, da, db)).astype(np.float64)
            else:
                d = np.abs(np.where(fin, t64, 0.0) - win(tp, da, db).astype(np.float64))
            dstep = np.where(win(hp, da, db) & (d > dstep), d, dstep)
        hi = np.full((na, nb), -np.inf, np.float32)
        lo = np.full((na, nb), np.inf, np.float32)
        support = np.zeros((na, nb), np.int64)
        fp = footprint(r2, square=variant == "square")
        for da, db in fp:
            g, t = win(hp, da, db), win(tp, da, db)
            hi = np.where(g & (t > hi), t, hi)
            lo = np.where(g & (t < lo), t, lo)
            support += win(gp, da, db)
        if variant == "f32_sub":
            drelief = np.where(hi > lo, hi - lo, np.float32(0)).astype(np.float64)
        else:
            drelief = np.where(hi > lo, hi.astype(np.float64) - lo.astype(np.float64), 0.0)
        a = ground & ((dstep >= prm.max_step) if variant == "step_ge" else (dstep > prm.max_step))
        b = ground & ((drelief >= prm.max_relief) if variant == "relief_ge" else (drelief > prm.max_relief))
        c = ground & (support * 256 < prm.min_support_256 * len(fp))
        step = np.where(ground, dstep.astype(np.float32), np.float32(-1))
        relief = np.where(ground, drelief.astype(np.float32), np.float32(-1))
    if variant == "rough_first":
        is_rough = b
        is_step = a & ~b
    else:
        is_step = a
        is_rough = b & ~a
    is_unsup = c & ~a & ~b
    kept = ground & ~a & ~b & ~c
    out = np.array(cls)
    out[is_step], out[is_rough], out[is_unsup] = STEP, ROUGH, UNSUPPORTED
    if variant != "nonfinite_through":
        out[nonfinite] = UNSUPPORTED
    counts = tuple(int(m.sum()) for m in (ground, is_step, is_rough, is_unsup, nonfinite, kept))
    s = Surface(out, step.astype(np.float32), relief.astype(np.float32), support.astype(np.uint16), counts)
    return (s, (a, b, c)) if detail else s


def same(x, y):
    return (np.array_equal(x.cls_out, y.cls_out) and np.array_equal(x.step.view(np.uint32), y.step.view(np.uint32)) and
            np.array_equal(x.relief.view(np.uint32), y.relief.view(np.uint32)) and np.array_equal(x.support, y.support) and
            tuple(x.counts) == tuple(y.counts))


def agrees_at(s, cells):
    """Whether the Surface s holds what surface_py gave for these cells."""
    return all((int(s.cls_out[k]), int(s.step.view(np.uint32)[k]), int(s.relief.view(np.uint32)[k]), int(s.support[k])) == v[:4]
               for k, v in cells.items())


def sample_cells(na, nb, count, seed=0):
    """The corners, the middles of the edges and seeded cells."""
    rng = np.random.default_rng([seed, na, nb])
    fixed = {(a, b) for a in (0, na // 2, na - 1) for b in (0, nb // 2, nb - 1)}
    return sorted(fixed | {(int(rng.integers(na)), int(rng.integers(nb))) for _ in range(count)})


# ------------------------------------------------------------------------------------------------ seeded random cases
def random_case(na, nb, seed=0, nonground=0.12, high=0.02, nonfinite=0.02):
    """cls and top: a smooth height field (three low-frequency waves, about 0.05 per cell at the steepest) with cliffs of 0.45 and of
    1.0 along seeded lines; `nonground` of the cells UNKNOWN (top -inf, as the grid writes it) or OBSTACLE (a finite top), `high` of
    them of a class 32 .. 255 (finite tops), `nonfinite` of them LEVEL with a top of NaN, +inf or -inf."""
    rng = np.random.default_rng([seed, na, nb])
    ia, ib = np.meshgrid(np.arange(na, dtype=np.float64), np.arange(nb, dtype=np.float64), indexing="ij")
    h = np.zeros((na, nb))
    for _ in range(3):
        fa, fb, ph = rng.uniform(-0.12, 0.12), rng.uniform(-0.12, 0.12), rng.uniform(0, 2 * np.pi)
        h += 0.25 * np.sin(fa * ia + fb * ib + ph)
    for height in (0.45, 1.0):
        ca, cb, th = rng.uniform(0, na), rng.uniform(0, nb), rng.uniform(0, np.pi)
        h += height * (((ia - ca) * np.cos(th) + (ib - cb) * np.sin(th)) > 0)
    top = h.astype(np.float32)
    cls = np.ones((na, nb), np.uint8)
    u = rng.uniform(size=(na, nb))
    unknown = u < nonground / 2
    obstacle = (u >= nonground / 2) & (u < nonground)
    hi = (u >= nonground) & (u < nonground + high)
    nf = (u >= nonground + high) & (u < nonground + high + nonfinite)
    cls[unknown], cls[obstacle] = 0, 2
    top[unknown] = -np.inf
    top[obstacle] += np.float32(0.8)
    cls[hi] = rng.integers(32, 256, size=int(hi.sum())).astype(np.uint8)
    top[nf] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), size=int(nf.sum()))
    return cls, top


SIZES = ((1, 1), (1, 40), (40, 1), (17, 17), (33, 31), (63, 65), (130, 300))
R2S = (0, 1, 2, 8, 25, 225)
RANDOM_SUPPORT = 200  # min_support_256 of the random cases: 78 % of the footprint


def random_params(cls, r2):
    return params(cls, r2, min_support_256=RANDOM_SUPPORT)


def seam_case():
    """Cliffs of 1.0 exactly between the rows 7|8, 15|16, 31|32 and the columns 15|16, 31|32, 63|64: the seams of every tile shape
    of 256 cells with sides 4 .. 64, in both directions, on ground that is otherwise flat."""
    na, nb = 40, 80
    ia, ib = np.meshgrid(np.arange(na), np.arange(nb), indexing="ij")
    top = sum((ia >= k).astype(np.float32) for k in (8, 16, 32)) + sum(4 * (ib >= k).astype(np.float32) for k in (16, 32, 64))
    return np.ones((na, nb), np.uint8), top.astype(np.float32)


# ------------------------------------------------------------------------------------------------ constructed grids
# max_step 0.35, not 0.3: the ramp's sides differ from the plateaus by multiples of 0.1f, and (double)0.3f > 0.3 is the business of
# another constructed pair, not of this one.  lane_rows: the ramp's two inner rows, whose every neighbour is ramp or the ramp's ends.
TERRACE = dict(na=12, nb=20, ledge=10, ramp_rows=(4, 8), ramp_cols=(5, 15), lane_rows=(5, 7), max_step=0.35)


def terrace_tops(ramp=True):
    """Two plateaus, 0 for ib < 10 and 1 for ib >= 10; across the ledge, in the rows 4 .. 7, a ramp over the columns 5 .. 14 that
    rises 0.1 per cell from 0.1 to 1.0."""
    t = TERRACE
    top = np.zeros((t["na"], t["nb"]), np.float32)
    top[:, t["ledge"]:] = 1.0
    if ramp:
        for ib in range(*t["ramp_cols"]):
            top[t["ramp_rows"][0]:t["ramp_rows"][1], ib] = np.float32(0.1 * (ib - 4))
    return top


def constructed():
    """name -> (cls, top, params): the facts each was built for are asserted in tests/test_grid_surface.py on the restatement alone."""
    f32 = lambda *v: np.array([v], np.float32)
    level = lambda top: np.ones(top.shape, np.uint8)
    g = {}
    top = terrace_tops()
    g["terrace"] = (level(top), top, params(top, 2, max_step=TERRACE["max_step"], max_relief=INF))
    top = (np.float32(0.25) * np.arange(40, dtype=np.float32))[None, :].repeat(9, axis=0)
    g["slope"] = (level(top), top, params(top, 25, max_step=0.3, max_relief=0.6))
    top = f32(0.0, 0.3)
    g["0.3f against (double)0.3f"] = (level(top), top, params(top, 0, max_step=F03, max_relief=INF))
    g["0.3f against 0.3"] = (level(top), top, params(top, 0, max_step=0.3, max_relief=INF))
    top = f32(0.0, 0.5)
    g["relief at the bound"] = (level(top), top, params(top, 1, max_step=INF, max_relief=0.5))
    top = f32(-0.0, 0.0)
    g["zeros"] = (level(top), top, params(top, 1, max_step=0.0, max_relief=0.0))
    top = f32(16777216.0, 1.0)
    g["big_exact"] = (level(top), top, params(top, 0, max_step=16777214.5, max_relief=INF))
    top = f32(16777216.0, -1.0)
    g["big_f32_wrong"] = (level(top), top, params(top, 0, max_step=16777216.0, max_relief=INF))
    cls = np.zeros((3, 3), np.uint8)
    cls[1, 1] = 1
    top = np.full((3, 3), -np.inf, np.float32)
    top[1, 1] = 0.0
    g["island"] = (cls, top, params(top, 2, min_support_256=128))
    g["across_an_obstacle"] = (np.array([[1, 2, 1]], np.uint8), f32(0.0, 0.5, 1.0), params(f32(0, 0, 0), 0, max_step=0.3, max_relief=INF))
    return g
