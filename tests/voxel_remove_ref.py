"""The removal's contract (include/svo.h, "Voxel map removal") restated twice, by two routes that share no code:

  remove_np   whole arrays: a cloud's contributions per key by voxel_ref.insert_np (np.unique and np.add.at), then item 3 as array
              operations on the table;
  remove_py   record by record in Python integers on the dict {key: [ci, sx, sy, sz]} that voxel_ref.insert_py builds, with a
              front half of its own.

Both return (Table, counts); a Table here keeps its zero-payload keys (a removal never takes a key out), and counts is
{n_removed, n_rejected, n_missing, n_short} in points.  `variant` of remove_np states one deliberate misreading of the contract
each.  Also here: the saturation scenes and the small helpers the GPU tests share.  Nothing here is tuned on the library's output.
"""
import math
from collections import namedtuple

import numpy as np

import voxel_ref as V

Table = namedtuple("Table", "keys ci sx sy sz")
COUNTS = ("n_removed", "n_rejected", "n_missing", "n_short")
VARIANTS = ("no_zeroing", "wrap", "claim", "isum_kept", "short_per_voxel")
LO40 = (1 << 40) - 1


def table_of(t):
    """A voxel_ref.Table (or one of ours) without its point counts."""
    return Table(t.keys, t.ci, t.sx, t.sy, t.sz)


def same(a, b):
    return all(np.array_equal(getattr(a, n), getattr(b, n)) for n in Table._fields)


def live(t):
    """The voxels with count > 0: what two maps that differ only in zero-payload keys have in common."""
    keep = (t.ci >> np.uint64(40)) > 0
    return Table(*(getattr(t, n)[keep] for n in Table._fields))


def as_dict(t):
    return {int(k): [int(c), int(x), int(y), int(z)] for k, c, x, y, z in zip(*(getattr(t, n).tolist() for n in Table._fields))}


def from_dict(d):
    ks = sorted(d)
    col = lambda j: np.array([d[k][j] for k in ks], np.uint64)
    return Table(np.array(ks, np.uint64), col(0), col(1), col(2), col(3))


# ------------------------------------------------------------------------------------------------ route (a): numpy
def remove_np(table, points, m12, voxel_size, max_depth=0.0, variant=None):
    c = V.insert_np(points, m12, voxel_size, max_depth)  # the cloud's contributions per key: (C << 40 | I, F_0, F_1, F_2)
    u64 = np.uint64
    pos = np.searchsorted(table.keys, c.keys)
    pos_c = np.minimum(pos, max(len(table.keys) - 1, 0))
    found = (table.keys[pos_c] == c.keys) if len(table.keys) else np.zeros(len(c.keys), bool)
    C, I = c.ci >> u64(40), c.ci & u64(LO40)
    n_missing = int(C[~found].sum())
    keys, words = table.keys, [w.copy() for w in (table.ci, table.sx, table.sy, table.sz)]
    if variant == "claim" and (~found).any():  # a removal that claims what it does not find
        keys = np.concatenate([keys, c.keys[~found]])
        o = np.argsort(keys)
        words = [np.concatenate([w, np.zeros(int((~found).sum()), u64)])[o] for w in words]
        keys = keys[o]
        pos, found = np.searchsorted(keys, c.keys), np.ones(len(c.keys), bool)
        n_missing = 0
    at = pos[found]
    C, I, F = C[found], I[found], [f[found] for f in (c.sx, c.sy, c.sz)]
    count, isum = words[0][at] >> u64(40), words[0][at] & u64(LO40)
    sat = lambda a, b: np.where(a > b, a - b, u64(0))
    if variant == "wrap":
        left = (count - C) & u64((1 << 24) - 1)
        isum2 = (isum - I) & u64(LO40)
        sums = [words[1 + r][at] - F[r] for r in range(3)]
    else:
        left = sat(count, C)
        isum2 = sat(isum, I)
        sums = [sat(words[1 + r][at], F[r]) for r in range(3)]
    gone = left == 0
    if variant not in ("no_zeroing", "wrap"):
        if variant != "isum_kept":
            isum2 = np.where(gone, u64(0), isum2)
        sums = [np.where(gone, u64(0), s) for s in sums]
    short = C - (count - sat(count, C))
    n_short = int((short > 0).sum()) if variant == "short_per_voxel" else int(short.sum())
    words[0][at] = (left << u64(40)) | isum2
    for r in range(3):
        words[1 + r][at] = sums[r]
    counts = dict(zip(COUNTS, (int(C.sum()), c.n_rejected, n_missing, n_short)))
    return Table(keys, *words), counts


# ------------------------------------------------------------------------------------------------ route (b): Python
def _record_py(px, py, pz, tag, m, vs, md):
    """(key, intensity, [f_0, f_1, f_2]) of one record, or None if it is rejected: items 1-3, one f64 operation per line."""
    if not (pz > 0.0) or (md > 0.0 and pz > md):
        return None
    key, fs = 0, []
    for r in range(3):
        w = m[4 * r] * px
        w = w + m[4 * r + 1] * py
        w = w + m[4 * r + 2] * pz
        w = w + m[4 * r + 3]
        q = w / vs
        if not (q >= -V.LIMIT and q < V.LIMIT):
            return None
        k = math.floor(q)
        fs.append(min(int(math.floor((q - k) * 65536.0)), 65535))
        key |= (k + (1 << 20)) << (21 * r)
    return key, tag >> 24, fs


def remove_py(vox, points, m12, voxel_size, max_depth=0.0):
    """vox: {key: [ci, sx, sy, sz]}, changed in place, one record after the other in the order given."""
    m = [float(v) for v in np.asarray(m12, np.float64).reshape(12)]
    vs, md = float(np.float32(voxel_size)), float(np.float32(max_depth))
    n = dict.fromkeys(COUNTS, 0)
    for px, py, pz, tag in points.tolist():
        rec = _record_py(px, py, pz, tag, m, vs, md)
        if rec is None:
            n["n_rejected"] += 1
            continue
        key, inten, fs = rec
        v = vox.get(key)
        if v is None:
            n["n_missing"] += 1
            continue
        n["n_removed"] += 1
        count, isum = v[0] >> 40, v[0] & LO40
        if count == 0:
            n["n_short"] += 1
            continue
        if count == 1:
            v[:] = [0, 0, 0, 0]
            continue
        v[0] = ((count - 1) << 40) | max(0, isum - inten)
        for r in range(3):
            v[1 + r] = max(0, v[1 + r] - fs[r])
    return from_dict(vox), n


def both(table, points, m12, voxel_size, max_depth=0.0):
    """The removal by both routes, asserted equal; returns the numpy route's result."""
    a, ca = remove_np(table, points, m12, voxel_size, max_depth)
    b, cb = remove_py(as_dict(table), points, m12, voxel_size, max_depth)
    assert same(a, b) and ca == cb, (ca, cb)
    assert ca["n_removed"] + ca["n_rejected"] + ca["n_missing"] == len(points)
    return a, ca


def insert(table, points, m12, voxel_size, max_depth=0.0):
    """The table after one more insert (zero-payload keys kept)."""
    t = V.insert_np(points, m12, voxel_size, max_depth)
    if table is None:
        return table_of(t)
    d = as_dict(table)
    for k, w in as_dict(t).items():
        v = d.setdefault(k, [0, 0, 0, 0])
        for j in range(4):
            v[j] += w[j]
    return from_dict(d)


# ------------------------------------------------------------------------------------------------ saturation scenes
IDENT = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64)


def in_voxel(cell, frac, inten):
    """Records in the voxel `cell` (integer coordinates at 0.25 m under the identity: q = 4 x exactly), at the fractions `frac`
    (n x 3, multiples of 1/256 in [0, 1)) of its edge, with the intensities `inten`."""
    frac = np.asarray(frac, np.float64).reshape(-1, 3)
    xyz = ((np.asarray(cell, np.float64) + frac) * 0.25).astype(np.float32)
    tag = (np.arange(len(frac), dtype=np.uint32) | (np.asarray(inten, np.uint32) << np.uint32(24))).astype(np.uint32)
    return V.records(xyz[:, 0], xyz[:, 1], xyz[:, 2], tag)


def filler(n, row=0):
    """n records in n distinct voxels of their own (row `row` of cells), far from CELL."""
    return np.concatenate([in_voxel((20 + i, row, 9), [(0.5, 0.5, 0.5)], [7]) for i in range(n)])


CELL = (3, -2, 8)
VS, LOG2 = 0.25, 8


def saturation_scenes():
    """name -> (inserted records, removed records, expected (count, isum, sx, sy, sz) of CELL afterwards, expected n_short)."""
    lo, hi = [(0.125, 0.25, 0.375)], [(0.75, 0.875, 0.9375)]
    out = {}
    # count 3; found contributions of 2 and 3 with a hundred other records between them: different wavefronts' heads meet the voxel
    three = in_voxel(CELL, lo * 3, [10, 20, 30])
    rm = np.concatenate([in_voxel(CELL, hi * 2, [1, 2]), filler(100), in_voxel(CELL, hi * 3, [3, 4, 5])])
    out["count_3_minus_2_and_3"] = (np.concatenate([three, filler(100)]), rm, (0, 0, 0, 0, 0), 2)
    # count 5 minus three OTHER records with larger fractions and intensities: count 2, every sum saturates at 0
    five = in_voxel(CELL, lo * 5, [10, 20, 30, 40, 50])
    out["count_5_minus_3_larger"] = (five, in_voxel(CELL, hi * 3, [250, 251, 252]), (2, 0, 0, 0, 0), 0)
    # count 5 minus 2 of its own: exact
    own = five[[1, 3]]
    out["count_5_minus_2_own"] = (five, own, (3, 10 + 30 + 50, 3 * 8192, 3 * 16384, 3 * 24576), 0)
    return out


def cell_key(cell):
    return sum((int(c) + (1 << 20)) << (21 * r) for r, c in enumerate(cell))


def payload(table, key):
    i = int(np.searchsorted(table.keys, np.uint64(key)))
    assert int(table.keys[i]) == key
    ci = int(table.ci[i])
    return (ci >> 40, ci & LO40, int(table.sx[i]), int(table.sy[i]), int(table.sz[i]))
