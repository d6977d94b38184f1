"""The voxel map's contract (include/svo.h, "voxel map") restated twice, by two routes that share no code:

  insert_np   whole arrays in numpy: f64 arithmetic one operation per ufunc (numpy never contracts), np.unique over the keys,
              np.add.at for the sums;
  insert_py   record by record in Python integers and floats, into a dict.

Both return a Table (keys ascending, the four payload words, the inserted / rejected point counts).  `variant` of insert_np states
one deliberate misreading of the contract each; tests/test_voxel_map.py shows that every one of them changes the main scene.
Also here: the extraction, the occupied slot set under the declared hash and probing, its longest cyclic run, and the scenes.
Nothing here is tuned on the library's output.
"""
import math
from collections import namedtuple

import numpy as np

EMPTY = (1 << 64) - 1
MAX_PROBES = 64
LIMIT = 1048576.0
M64 = (1 << 64) - 1
POINT = np.dtype([("x", np.float32), ("y", np.float32), ("z", np.float32), ("tag", np.uint32)])
Table = namedtuple("Table", "keys ci sx sy sz n_inserted n_rejected")


def records(x, y, z, tag):
    p = np.empty(len(x), POINT)
    p["x"], p["y"], p["z"], p["tag"] = x, y, z, tag
    return p


# ------------------------------------------------------------------------------------------------ route (a): numpy
def insert_np(points, m12, voxel_size, max_depth=0.0, variant=None):
    m = np.asarray(m12, np.float64).reshape(3, 4)
    vs = np.float64(np.float32(voxel_size))
    md = np.float32(max_depth)
    z32 = points["z"]
    with np.errstate(all="ignore"):
        ok = (z32 >= np.float32(0)) if variant == "z_ge_0" else (z32 > np.float32(0))
        if md > 0:
            ok &= ~(z32 > md)
        x, y, z = (points[c].astype(np.float64) for c in "xyz")
        q = []
        for r in range(3):
            w = m[r, 0] * x
            w = w + m[r, 1] * y
            w = w + m[r, 2] * z
            w = w + m[r, 3]
            if variant == "w_f32":
                w = w.astype(np.float32).astype(np.float64)
            qr = w / vs
            ok &= (qr >= -LIMIT) & (qr < LIMIT)
            q.append(qr)
    n_rejected = int((~ok).sum())
    q = [qr[ok] for qr in q]
    tag = points["tag"][ok]
    key = np.zeros(len(tag), np.uint64)
    f = []
    for r in range(3):
        k = np.trunc(q[r]) if variant == "trunc" else np.floor(q[r])
        fr = np.floor((q[r] - k) * (65535.0 if variant == "scale_65535" else 65536.0))
        if variant == "trunc":
            fr = np.abs(fr)  # a truncating implementation has no negative fraction to store either
        fr = fr.astype(np.uint64)
        f.append(fr if variant == "no_clamp" else np.minimum(fr, np.uint64(65535)))
        key |= (k.astype(np.int64) + (1 << 20)).astype(np.uint64) << np.uint64(21 * r)
    inten = (tag & np.uint32(0xFF)) if variant == "tag_low_byte" else (tag >> np.uint32(24))
    keys, inv = np.unique(key, return_inverse=True)
    out = [np.zeros(len(keys), np.uint64) for _ in range(4)]
    np.add.at(out[0], inv, (np.uint64(1) << np.uint64(40)) | inten.astype(np.uint64))
    for r in range(3):
        np.add.at(out[1 + r], inv, f[r])
    return Table(keys, out[0], out[1], out[2], out[3], int(ok.sum()), n_rejected)


# ------------------------------------------------------------------------------------------------ route (b): Python
def insert_py(points, m12, voxel_size, max_depth=0.0, into=None):
    """into: a dict of an earlier call to go on with (accumulation); returned as Table.  The dict is in Table-less form
    key -> [ci, sx, sy, sz] under insert_py.last."""
    m = [float(v) for v in np.asarray(m12, np.float64).reshape(12)]
    vs = float(np.float32(voxel_size))
    md = float(np.float32(max_depth))
    vox = {} if into is None else into
    n_ins = n_rej = 0
    for px, py, pz, tag in points.tolist():
        if not (pz > 0.0) or (md > 0.0 and pz > md):
            n_rej += 1
            continue
        key, fs, good = 0, [], True
        for r in range(3):
            w = m[4 * r] * px
            w = w + m[4 * r + 1] * py
            w = w + m[4 * r + 2] * pz
            w = w + m[4 * r + 3]
            q = w / vs
            if not (q >= -LIMIT and q < LIMIT):
                good = False
                break
            k = math.floor(q)
            fs.append(min(int(math.floor((q - k) * 65536.0)), 65535))
            key |= (k + (1 << 20)) << (21 * r)
        if not good:
            n_rej += 1
            continue
        n_ins += 1
        v = vox.setdefault(key, [0, 0, 0, 0])
        v[0] += (1 << 40) | (tag >> 24)
        for r in range(3):
            v[1 + r] += fs[r]
    insert_py.last = vox
    ks = sorted(vox)
    col = lambda j: np.array([vox[k][j] for k in ks], np.uint64)
    return Table(np.array(ks, np.uint64), col(0), col(1), col(2), col(3), n_ins, n_rej)


def same(a, b):
    return all(np.array_equal(getattr(a, n), getattr(b, n)) for n in ("keys", "ci", "sx", "sy", "sz")) and \
        (a.n_inserted, a.n_rejected) == (b.n_inserted, b.n_rejected)


def merge(a, b):
    """The table after both insertions (keys united, payload words and counts added)."""
    d = {}
    for t in (a, b):
        for k, c, x, y, z in zip(*(v.tolist() for v in (t.keys, t.ci, t.sx, t.sy, t.sz))):
            v = d.setdefault(k, [0, 0, 0, 0])
            v[0] += c; v[1] += x; v[2] += y; v[3] += z
    ks = sorted(d)
    col = lambda j: np.array([d[k][j] for k in ks], np.uint64)
    return Table(np.array(ks, np.uint64), col(0), col(1), col(2), col(3), a.n_inserted + b.n_inserted, a.n_rejected + b.n_rejected)


def changed_voxels(a, b):
    """How many voxels differ between two tables: keys in one only, plus common keys whose payload differs."""
    da = {int(k): (int(c), int(x), int(y), int(z)) for k, c, x, y, z in zip(a.keys, a.ci, a.sx, a.sy, a.sz)}
    db = {int(k): (int(c), int(x), int(y), int(z)) for k, c, x, y, z in zip(b.keys, b.ci, b.sx, b.sy, b.sz)}
    return len(set(da) ^ set(db)) + sum(1 for k in set(da) & set(db) if da[k] != db[k])


# ------------------------------------------------------------------------------------------------ extraction
def extract(table, voxel_size, min_count=1):
    """The records of every voxel with count >= min_count, sorted by their bytes."""
    vs = float(np.float32(voxel_size))
    out = []
    for key, ci, sx, sy, sz in zip(*(a.tolist() for a in (table.keys, table.ci, table.sx, table.sy, table.sz))):
        count, isum = ci >> 40, ci & ((1 << 40) - 1)
        if count < min_count:
            continue
        c = float(count) * 65536.0
        xyz = [np.float32((float(((key >> (21 * r)) & 0x1FFFFF) - (1 << 20)) + float(s) / c) * vs) for r, s in enumerate((sx, sy, sz))]
        out.append((xyz[0], xyz[1], xyz[2], (count | ((isum // count) << 24)) & 0xFFFFFFFF))
    return sort_records(np.array(out, POINT) if out else np.empty(0, POINT))


def sort_records(p):
    b = np.ascontiguousarray(p).view(np.uint32).reshape(-1, 4)
    return b[np.lexsort(b.T[::-1])]


# ------------------------------------------------------------------------------------------------ hash and probing
def fmix64(k):
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & M64
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & M64
    k ^= k >> 33
    return k


def occupied(keys, capacity_log2):
    """The slots occupied after inserting these distinct keys by linear probing WITHOUT a probe bound, as a bool array.  The set
    does not depend on the insertion order."""
    cap = 1 << capacity_log2
    occ = np.zeros(cap, bool)
    assert len(keys) <= cap
    for k in np.asarray(keys, np.uint64).tolist():
        h = fmix64(k) & (cap - 1)
        while occ[h]:
            h = (h + 1) & (cap - 1)
        occ[h] = True
    return occ


def longest_run(occ):
    """The longest cyclic run of occupied slots.  Below MAX_PROBES no insertion order can drop a point: a probe sequence lies
    inside one run of the final occupied set, so it meets at most that many foreign slots."""
    if occ.all():
        return len(occ)
    s = int(np.argmin(occ))  # start behind a free slot: no run wraps
    best = cur = 0
    for v in np.roll(occ, -s).tolist():
        cur = cur + 1 if v else 0
        best = max(best, cur)
    return best


# ------------------------------------------------------------------------------------------------ scenes
def scene(width=160, height=80, seed=10):
    """A slanted plane (left half, 3.5 m to 12 m) beside a fronto-parallel one (right half, 4 m), through an ideal pinhole
    pair in numpy: disparity in sixteenths with 0..3 sixteenths of noise, then the usual triangulation in f32.  One pixel covers
    z / f = 2.9 cm to 10 cm, so at 0.05 .. 0.25 m voxels the scene runs from one to many pixels per voxel.  Every 97th pixel is a
    hole (a rejected record {0, 0, 0}: it separates runs), and the row through the optical axis has y = -1e-30f: under a
    transform whose y row is [0 1 0 0] its q_1 is a tiny negative number, the case the clamp of f exists for."""
    rng = np.random.default_rng(seed)
    f, b, cx, cy = 120.0, 0.5, width / 2.0, height / 2.0
    u, v = np.meshgrid(np.arange(width), np.arange(height))
    depth = np.where(u < width // 2, 3.5 + 8.5 * u / (width // 2), 4.0)
    d16 = np.floor(16.0 * f * b / depth) + rng.integers(0, 4, size=depth.shape)
    d = (d16 / 16.0).astype(np.float32)
    z = (np.float32(f * b) / d).astype(np.float32)
    x = ((u - cx).astype(np.float32) * z / np.float32(f)).astype(np.float32)
    y = ((v - cy).astype(np.float32) * z / np.float32(f)).astype(np.float32)
    y[v == int(cy)] = np.float32(-1e-30)
    inten = rng.integers(0, 256, size=depth.shape).astype(np.uint32)
    tag = (v * width + u).astype(np.uint32) | (inten << np.uint32(24))
    p = records(x.ravel(), y.ravel(), z.ravel(), tag.ravel())
    hole = np.arange(len(p)) % 97 == 96
    p["x"][hole] = p["y"][hole] = p["z"][hole] = 0
    return p


def rot_y(angle, shift):
    """Camera->world: a rotation about y and a shift, as 12 doubles (3 x 4 row-major)."""
    c, s = math.cos(angle), math.sin(angle)
    return np.array([c, 0, s, shift[0], 0, 1, 0, shift[1], -s, 0, c, shift[2]], np.float64)


def pose7_matrix(pose7):
    """[R(q)^T | -R(q)^T t] for pose7 = [qw qx qy qz tx ty tz] (X_cam = R(q) X_world + t), through numpy's matrix product of the
    textbook rotation of the NORMALISED quaternion: another route than the library's s = 2 / |q|^2 form."""
    q = np.asarray(pose7[:4], np.float64)
    w, x, y, z = q / np.linalg.norm(q)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    t = np.asarray(pose7[4:], np.float64)
    return np.hstack([R.T, (-R.T @ t)[:, None]])


def run_heads(points, m12, voxel_size, max_depth=0.0):
    """How many lanes would probe: records whose key differs from the record before them inside their 64-record wavefront (or
    that open one), rejected records aside.  A figure for reports, never compared with the library."""
    m = np.asarray(m12, np.float64).reshape(3, 4)
    vs = np.float64(np.float32(voxel_size))
    with np.errstate(all="ignore"):
        ok = points["z"] > 0
        if max_depth > 0:
            ok &= ~(points["z"] > np.float32(max_depth))
        x, y, z = (points[c].astype(np.float64) for c in "xyz")
        key = np.zeros(len(points), np.uint64)
        for r in range(3):
            q = (((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3]) / vs
            ok &= (q >= -LIMIT) & (q < LIMIT)
            key |= (np.floor(np.where(ok, q, 0.0)).astype(np.int64) + (1 << 20)).astype(np.uint64) << np.uint64(21 * r)
    key[~ok] = np.uint64(EMPTY)
    first = np.ones(len(key), bool)
    first[1:] = key[1:] != key[:-1]
    first[::64] = True
    return int((first & ok).sum())
