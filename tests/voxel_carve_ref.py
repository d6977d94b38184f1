"""Free-space carving and the copy of the live voxels (include/svo.h, "Free-space carving") restated twice, by two
routes that share no code, on the Tables of tests/voxel_ref.py (keys ascending, four payload words; a carved voxel keeps its key
and has four zero words):

  carve_np   whole arrays in numpy, one f64 operation per ufunc (numpy never contracts);
  carve_py   slot by slot in Python floats and integers.

Both return (Table, (n_live, n_tested, n_carved)).  `variant` of carve_np states one deliberate misreading of the contract each;
tests/test_voxel_carve.py shows that every one of them changes the main scene's carved set.  Also here: the copy (filter, then
voxel_ref.merge), world->camera from a pose7 by another route than the library's, and the scenes.  Nothing here is tuned on the
library's output.
"""
import math

import numpy as np

import voxel_ref as V

FILTERED = -16
VARIANTS = ("centre", "le", "trunc", "voxel_centre", "invalid_as_zero", "keep_gt")


def _table(t, ci, sx, sy, sz):
    return V.Table(t.keys, ci, sx, sy, sz, t.n_inserted, t.n_rejected)


# ------------------------------------------------------------------------------------------------ route (a): numpy
def carve_np(table, disp16, cam, m12, voxel_size, radius=1, margin16=8, keep_count=0, variant=None):
    """cam = (focal, cx, cy, baseline); m12: world->camera, 12 doubles; disp16: (height, width) int16."""
    focal, cx, cy, baseline = (np.float64(v) for v in cam)
    m = np.asarray(m12, np.float64).reshape(3, 4)
    vs = np.float64(np.float32(voxel_size))
    disp = np.asarray(disp16, np.int16).astype(np.int64)
    H, W = disp.shape
    count = table.ci >> np.uint64(40)
    live = count >= np.uint64(1)
    with np.errstate(all="ignore"):
        c = count.astype(np.float64) * 65536.0
        p = []
        for r, s in enumerate((table.sx, table.sy, table.sz)):
            k = (((table.keys >> np.uint64(21 * r)) & np.uint64(0x1FFFFF)).astype(np.int64) - (1 << 20)).astype(np.float64)
            if variant == "voxel_centre":
                pr = k + 0.5
            else:
                pr = s.astype(np.float64) / c
                pr = k + pr
            p.append(pr * vs)
        q = []
        for r in range(3):
            w = m[r, 0] * p[0]
            w = w + m[r, 1] * p[1]
            w = w + m[r, 2] * p[2]
            q.append(w + m[r, 3])
        front = q[2] > 0.0
        pix = []
        for cr, centre in ((q[0], cx), (q[1], cy)):
            u = focal * cr
            u = u / q[2]
            u = u + centre
            pix.append(np.trunc(u) if variant == "trunc" else np.floor(u + 0.5))
        tested = live & front & (pix[0] >= radius) & (pix[0] <= W - 1 - radius) & (pix[1] >= radius) & (pix[1] <= H - 1 - radius)
        px = np.where(tested, pix[0], radius).astype(np.int64)
        py = np.where(tested, pix[1], radius).astype(np.int64)
        win = np.stack([disp[py + dy, px + dx] for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1)])
        evidence = (win > 0).all(0)
        dmax = win.max(0)
        if variant == "centre":
            dmax = disp[py, px]
        if variant == "invalid_as_zero":
            evidence = np.ones_like(evidence)
            dmax = np.maximum(win, 0).max(0)
        dv16 = focal * baseline
        dv16 = dv16 / q[2]
        dv16 = dv16 * 16.0
        lhs = (dmax + margin16).astype(np.float64)
        see = (lhs <= dv16) if variant == "le" else (lhs < dv16)
    kc = np.uint64(keep_count)
    protected = (keep_count > 0) & ((count > kc) if variant == "keep_gt" else (count >= kc))
    carved = tested & evidence & see & ~protected
    out = [np.where(carved, np.uint64(0), w) for w in (table.ci, table.sx, table.sy, table.sz)]
    return _table(table, *out), (int(live.sum()), int(tested.sum()), int(carved.sum()))


# ------------------------------------------------------------------------------------------------ route (b): Python
def carve_py(table, disp16, cam, m12, voxel_size, radius=1, margin16=8, keep_count=0):
    focal, cx, cy, baseline = (float(v) for v in cam)
    m = [float(v) for v in np.asarray(m12, np.float64).reshape(12)]
    vs = float(np.float32(voxel_size))
    rows = np.asarray(disp16, np.int16).tolist()
    H, W = len(rows), len(rows[0])
    cols = [a.tolist() for a in (table.keys, table.ci, table.sx, table.sy, table.sz)]
    n_live = n_tested = n_carved = 0
    for i, (key, ci, sx, sy, sz) in enumerate(zip(*cols)):
        count = ci >> 40
        if count < 1:
            continue
        n_live += 1
        pw = []
        for r, s in enumerate((sx, sy, sz)):
            k = ((key >> (21 * r)) & 0x1FFFFF) - (1 << 20)
            pw.append((float(k) + float(s) / (float(count) * 65536.0)) * vs)
        c = []
        for r in range(3):
            w = m[4 * r] * pw[0]
            w = w + m[4 * r + 1] * pw[1]
            w = w + m[4 * r + 2] * pw[2]
            c.append(w + m[4 * r + 3])
        if not c[2] > 0.0:
            continue
        u = focal * c[0] / c[2] + cx + 0.5
        v = focal * c[1] / c[2] + cy + 0.5
        if not (math.isfinite(u) and math.isfinite(v)):  # floor keeps an infinity or a NaN, and every comparison below fails on it
            continue
        px, py = math.floor(u), math.floor(v)
        if not (radius <= px <= W - 1 - radius and radius <= py <= H - 1 - radius):
            continue
        n_tested += 1
        dmax, evidence = None, True
        for y in range(py - radius, py + radius + 1):
            for x in range(px - radius, px + radius + 1):
                d = rows[y][x]
                if d <= 0:
                    evidence = False
                dmax = d if dmax is None or d > dmax else dmax
        if not evidence:
            continue
        dv16 = focal * baseline / c[2] * 16.0
        if not float(dmax + margin16) < dv16:
            continue
        if keep_count > 0 and count >= keep_count:
            continue
        for col in cols[1:]:
            col[i] = 0
        n_carved += 1
    u64 = lambda a: np.array(a, np.uint64)
    return _table(table, u64(cols[1]), u64(cols[2]), u64(cols[3]), u64(cols[4])), (n_live, n_tested, n_carved)


def carved_set(before, after):
    """The keys whose voxel was live before and is not after."""
    was = (before.ci >> np.uint64(40)) >= np.uint64(1)
    now = (after.ci >> np.uint64(40)) >= np.uint64(1)
    return set(before.keys[was & ~now].tolist())


# ------------------------------------------------------------------------------------------------ the copy
def copy_live(table, voxel_size, min_count=1, box=None):
    """The slots a copy moves: count >= min_count and, with box = (lo_x, lo_y, lo_z, hi_x, hi_y, hi_z), floor(lo_r / vs) <= k_r <=
    floor(hi_r / vs).  voxel_ref.merge(dst, copy_live(src, ...)) is dst after the copy; its n_inserted is what moved."""
    keep = (table.ci >> np.uint64(40)) >= np.uint64(min_count)
    if box is not None:
        vs = float(np.float32(voxel_size))
        for r in range(3):
            k = ((table.keys >> np.uint64(21 * r)) & np.uint64(0x1FFFFF)).astype(np.int64) - (1 << 20)
            keep &= (k >= _face(float(box[r]) / vs)) & (k <= _face(float(box[3 + r]) / vs))
    moved = int((table.ci[keep] >> np.uint64(40)).sum())
    return V.Table(table.keys[keep], table.ci[keep], table.sx[keep], table.sy[keep], table.sz[keep], moved, 0)


def _face(q):
    """floor(q); an infinite bound lies beyond every key (|k| <= 2^20)."""
    return math.floor(min(max(q, -2097152.0), 2097152.0))


def empty_table():
    z = np.empty(0, np.uint64)
    return V.Table(z, z, z, z, z, 0, 0)


# ------------------------------------------------------------------------------------------------ poses
def world_to_cam(pose7):
    """[R(q) | t] for pose7 = [qw qx qy qz tx ty tz] through the textbook rotation of the NORMALISED quaternion as a product of
    quaternions (v' = q v q*): another route than the library's s = 2 / |q|^2 form."""
    q = np.asarray(pose7[:4], np.float64)
    q = q / np.linalg.norm(q)

    def mul(a, b):
        return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                         a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                         a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
                         a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])

    conj = q * np.array([1.0, -1.0, -1.0, -1.0])
    R = np.stack([mul(mul(q, np.array([0.0, *e])), conj)[1:] for e in np.eye(3)], 1)
    return np.hstack([R, np.asarray(pose7[4:], np.float64)[:, None]])


# ------------------------------------------------------------------------------------------------ scenes
W, H = 160, 80
CAM = (120.0, 80.0, 40.0, 0.5)  # focal, cx, cy, baseline
VIEW_A, VIEW_B = (0.0, 0.0, 0.0), (0.35, 0.1, 0.0)
PATCH = (slice(30, 40), slice(84, 88))  # rows, columns of view B set to FILTERED: 4 x 10, over the box's right edge as B sees it
ZERO_PIXEL = (20, 60)                   # row, column of view B set to 0, inside the box as B sees it


def render(centre, with_box, seed):
    """The main scene from a camera at `centre` looking along +z, every plane fronto-parallel, so a per-pixel ray test renders it
    exactly: wall at z = 8, panel at z = 5 for world x < -1, box at z = 3 for |x| < 0.5, |y| < 0.45.  d16 = floor(16 f B / z) +
    noise 0..2.  Returns (disp16 (H, W) int16, is_box (H, W) bool)."""
    f, cx, cy, b = CAM
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    dx, dy = (u - cx) / f, (v - cy) / f
    z = np.full((H, W), 8.0)
    z[centre[0] + 5.0 * dx < -1.0] = 5.0
    box = np.zeros((H, W), bool)
    if with_box:
        box = (np.abs(centre[0] + 3.0 * dx) < 0.5) & (np.abs(centre[1] + 3.0 * dy) < 0.45)
        z[box] = 3.0
    d16 = np.floor(16.0 * f * b / z) + rng.integers(0, 3, size=z.shape)
    return d16.astype(np.int16), box


def cloud(disp16, seed):
    """The cloud of a map in its camera frame, f32 as the library's clouds: d = d16 / 16, z = f B / d, x = (u - cx) z / f."""
    f, cx, cy, b = (np.float32(c) for c in CAM)
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    d = (disp16.astype(np.float32) / np.float32(16)).astype(np.float32)
    z = (f * b / d).astype(np.float32)
    x = ((u.astype(np.float32) - cx) * z / f).astype(np.float32)
    y = ((v.astype(np.float32) - cy) * z / f).astype(np.float32)
    inten = rng.integers(0, 256, size=z.shape).astype(np.uint32)
    tag = (v * W + u).astype(np.uint32) | (inten << np.uint32(24))
    return V.records(x.ravel(), y.ravel(), z.ravel(), tag.ravel())


def shift(centre, to_world):
    """12 doubles for a camera at `centre` without rotation: camera->world [I | centre] or world->camera [I | -centre]."""
    s = 1.0 if to_world else -1.0
    return np.array([1, 0, 0, s * centre[0], 0, 1, 0, s * centre[1], 0, 0, 1, s * centre[2]], np.float64)


def main_scene():
    """(cloud of view A, map of view A, is-box flags of A's pixels, map of view B with its FILTERED patch and its zero pixel)."""
    da, box = render(VIEW_A, True, 20)
    db, _ = render(VIEW_B, False, 21)
    db[PATCH] = FILTERED
    db[ZERO_PIXEL] = 0
    return cloud(da, 22), da, box.ravel(), db
