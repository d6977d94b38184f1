"""The voxel map normals and the plane form of the align (include/svo.h, "Voxel map normals" and "Voxel map align, plane form";
DESIGN 7r) restated by two routes that share no code:

  normals_np / plane_sums_np   whole arrays in numpy: f64 arithmetic one operation per ufunc (numpy never contracts), int64 moments,
                               the 27 candidates as an (n, 27) key array looked up in a sorted list of the reachable slots, the
                               Jacobi with np.where for the skipped pairs, the words summed with np.add.reduce on int64.  The
                               matching of the plane sums (rules 1-3 of the align) is voxel_align_ref.sums_np's, by import;
  normals_py / plane_sums_py   slot by slot and record by record in Python ints and floats, probing the raw downloaded table.

Both take the table in the download's form (a dict of uint64 arrays "keys", "ci", "sx", "sy", "sz").  The normals come back as an
array of NORMAL records, one per slot, and the 8 counts; the plane sums as 40 Python ints.  `variant` of the numpy routes states one
deliberate misreading of the contract each.  plane_loop() restates the host loop once, in Python floats, with voxel_align_ref's
solve, update, from_pose7, matrix and to_pose7 by import.  Nothing here is tuned on the library's output.
"""
import math
from collections import namedtuple

import numpy as np

import voxel_align_ref as A
import voxel_ref as V

NORMAL = np.dtype([("nx", np.float32), ("ny", np.float32), ("nz", np.float32), ("curvature", np.float32)])
COUNTS = ("n_centres", "n_valid", "n_few", "n_collinear", "n_curved")
N_COUNTS = 8
SWEEPS = 4
PLANE_WORDS = 40
PLANE_COUNTS = ("n_matched", "n_rejected", "n_unmatched", "n_far", "n_no_normal")
S20, S28, S30, S36, S40 = 2.0 ** 20, 2.0 ** 28, 2.0 ** 30, 2.0 ** 36, 2.0 ** 40
VARIANTS = ("count_weighted", "no_factor_n", "float_mean", "three_sweeps", "no_sign_rule", "curv_lt", "no_centre")
PLANE_VARIANTS = ("r_camera", "cross_sign", "one_scale", "nearest_with_normal")
Params = namedtuple("Params", "min_count min_neighbours max_curvature")
FIELD = 0x1FFFFF
PAIRS = ((0, 1, 2), (0, 2, 1), (1, 2, 0))  # (p, q, the third index)


def default_params(**over):
    return Params(1, 5, 1.0)._replace(**over)


def none_records(n):
    out = np.zeros(n, NORMAL)
    out["curvature"] = np.float32(-1.0)
    return out


def bits(normals):
    """The records as an (n, 4) array of their bit patterns."""
    return np.ascontiguousarray(normals).view(np.uint32).reshape(-1, 4)


def by_key(d, normals):
    """key -> the four bit patterns of its record, for every occupied slot."""
    at = np.flatnonzero(d["keys"] != np.uint64(V.EMPTY))
    b = bits(normals)
    return {int(d["keys"][i]): tuple(b[i].tolist()) for i in at.tolist()}


# ------------------------------------------------------------------------------------------------ route (a): numpy
def _reachable(d):
    cap = len(d["keys"])
    at = np.flatnonzero(d["keys"] != np.uint64(V.EMPTY))
    home = np.array([V.fmix64(k) & (cap - 1) for k in d["keys"][at].tolist()], np.int64)
    at = at[((at - home) & (cap - 1)) < V.MAX_PROBES]
    return at[np.argsort(d["keys"][at])]


def _lookup(d, key):
    """(found, slot) of every key of the array; the slot of a key that is not found is 0."""
    at = _reachable(d)
    tk = d["keys"][at]
    if not len(tk):
        return np.zeros(key.shape, bool), np.zeros(key.shape, np.int64)
    pos = np.minimum(np.searchsorted(tk, key), len(tk) - 1)
    found = tk[pos] == key
    return found, np.where(found, at[pos], 0)


def _jacobi_np(C, sweeps):
    """C: dict (r, s) -> int64 array, r <= s.  Returns (lambda as 3 arrays, V as 3 x 3 arrays)."""
    a = {rs: c.astype(np.float64) for rs, c in C.items()}
    n = len(a[(0, 0)])
    v = [[np.full(n, 1.0 if i == j else 0.0) for j in range(3)] for i in range(3)]
    g = lambda i, j: a[(min(i, j), max(i, j))]

    def put(i, j, val):
        a[(min(i, j), max(i, j))] = val

    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p, q, r in PAIRS:
                apq, app, aqq = g(p, q), g(p, p), g(q, q)
                skip = apq == 0.0
                th = (aqq - app) / (2.0 * apq)
                t = np.where(th >= 0.0, 1.0, -1.0) / (np.abs(th) + np.sqrt(th * th + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                x = t * apq
                put(p, p, np.where(skip, app, app - x))
                put(q, q, np.where(skip, aqq, aqq + x))
                put(p, q, np.where(skip, apq, 0.0))
                y, z = g(r, p), g(r, q)
                put(r, p, np.where(skip, y, c * y - s * z))
                put(r, q, np.where(skip, z, s * y + c * z))
                for k in range(3):
                    y, z = v[k][p], v[k][q]
                    v[k][p] = np.where(skip, y, c * y - s * z)
                    v[k][q] = np.where(skip, z, s * y + c * z)
    return [a[(0, 0)], a[(1, 1)], a[(2, 2)]], v


def normals_np(d, prm, variant=None):
    cap = len(d["keys"])
    out = none_records(cap)
    count_all = d["ci"] >> np.uint64(40)
    centres = np.flatnonzero((d["keys"] != np.uint64(V.EMPTY)) & (count_all >= np.uint64(prm.min_count)))
    counts = [len(centres), 0, 0, 0, 0, 0, 0, 0]
    if not len(centres):
        return out, counts
    key = d["keys"][centres]
    off = np.array(A.offsets(1), np.int64)  # (27, 3)
    idx = [((key >> np.uint64(21 * r)) & np.uint64(FIELD)).astype(np.int64)[:, None] + off[None, :, r] for r in range(3)]  # fields, 0..2^21-1 in range
    inr = np.ones(idx[0].shape, bool)
    ckey = np.zeros(idx[0].shape, np.uint64)
    for r in range(3):
        inr &= (idx[r] >= 0) & (idx[r] <= FIELD)
        ckey |= np.where(inr, idx[r], 0).astype(np.uint64) << np.uint64(21 * r)
    found, slot = _lookup(d, ckey)
    found &= inr
    cnt = np.where(found, count_all[slot], np.uint64(0))
    part = found & (cnt >= np.uint64(prm.min_count))
    # the centre takes part as the slot it is, wherever in its probe run it sits
    slot[:, 13] = centres
    cnt[:, 13] = count_all[centres]
    part[:, 13] = variant != "no_centre"
    c1 = np.where(part, cnt, np.uint64(1))
    g = []
    for r, name in enumerate(("sx", "sy", "sz")):
        if variant == "float_mean":
            g.append(off[None, :, r] * 65536.0 + d[name][slot].astype(np.float64) / c1.astype(np.float64))
        else:
            g.append(off[None, :, r] * 65536 + (d[name][slot] // c1).astype(np.int64))
    zero = 0.0 if variant == "float_mean" else 0
    wgt = np.where(part, cnt.astype(np.int64), 0) if variant == "count_weighted" else part.astype(np.int64)
    N = np.add.reduce(wgt, axis=1)
    n_part = np.add.reduce(part.astype(np.int64), axis=1)
    S1 = [np.add.reduce(np.where(part, wgt * g[r], zero), axis=1) for r in range(3)]
    C = {}
    for r in range(3):
        for s in range(r, 3):
            S2 = np.add.reduce(np.where(part, wgt * (g[r] * g[s]), zero), axis=1)
            C[(r, s)] = (S2 if variant == "no_factor_n" else N * S2) - S1[r] * S1[s]
    lam, v = _jacobi_np(C, 3 if variant == "three_sweeps" else SWEEPS)
    L = np.stack(lam, axis=1)
    lo = np.argmin(L, axis=1)  # the first of equal minima
    rows = np.arange(len(lo))
    l_lo = L[rows, lo]
    rest = np.where(np.arange(3)[None, :] == lo[:, None], np.inf, L)
    l_mid = rest.min(axis=1)
    tr = lam[0] + lam[1]
    tr = tr + lam[2]
    low = np.where(l_lo > 0.0, l_lo, 0.0)
    bound = np.float64(np.float32(prm.max_curvature)) * tr
    few = n_part < prm.min_neighbours
    collinear = ~few & ~(l_mid > 0.0)
    curved = ~few & ~collinear & ~((low < bound) if variant == "curv_lt" else (low <= bound))
    valid = ~few & ~collinear & ~curved
    nrm = [np.stack(v[k], axis=1)[rows, lo] for k in range(3)]
    mag = np.stack([np.abs(c) for c in nrm], axis=1)
    lead = np.stack(nrm, axis=1)[rows, np.argmax(mag, axis=1)]  # the first of equal maxima
    flip = (lead < 0.0) & (variant != "no_sign_rule")
    with np.errstate(all="ignore"):
        curv = low / tr
    at = centres[valid]
    for name, c in zip(("nx", "ny", "nz"), nrm):
        out[name][at] = np.where(flip, -c, c)[valid].astype(np.float32)
    out["curvature"][at] = curv[valid].astype(np.float32)
    counts[1:5] = [int(valid.sum()), int(few.sum()), int(collinear.sum()), int(curved.sum())]
    return out, counts


# ------------------------------------------------------------------------------------------------ route (b): Python
def _find(d, key):
    keys = d["keys"]
    cap = len(keys)
    h = V.fmix64(key) & (cap - 1)
    for _ in range(V.MAX_PROBES):
        k = int(keys[h])
        if k == key:
            return h
        if k == V.EMPTY:
            return -1
        h = (h + 1) & (cap - 1)
    return -1


def jacobi_py(C):
    """C: 3 x 3 nested lists of Python ints (symmetric).  Returns (lambda, V) in Python floats."""
    a = [[float(C[i][j]) for j in range(3)] for i in range(3)]
    v = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    for _ in range(SWEEPS):
        for p, q, r in PAIRS:
            apq = a[p][q]
            if apq == 0.0:
                continue
            th = (a[q][q] - a[p][p]) / (2.0 * apq)
            t = (1.0 if th >= 0.0 else -1.0) / (abs(th) + math.sqrt(th * th + 1.0))  # a product that overflows is inf, and t is 0
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            x = t * apq
            a[p][p] = a[p][p] - x
            a[q][q] = a[q][q] + x
            a[p][q] = a[q][p] = 0.0
            y, z = a[r][p], a[r][q]
            a[r][p] = a[p][r] = c * y - s * z
            a[r][q] = a[q][r] = s * y + c * z
            for k in range(3):
                y, z = v[k][p], v[k][q]
                v[k][p] = c * y - s * z
                v[k][q] = s * y + c * z
    return [a[0][0], a[1][1], a[2][2]], v


def record_py(parts, prm):
    """parts: the participants as (offset, count, (sx, sy, sz)).  Returns (the record as 4 floats or None, the verdict 0..3)."""
    N = len(parts)
    if N < prm.min_neighbours:
        return None, 1
    gs = [[o[r] * 65536 + s[r] // count for r in range(3)] for o, count, s in parts]
    S1 = [sum(g[r] for g in gs) for r in range(3)]
    C = [[N * sum(g[r] * g[s] for g in gs) - S1[r] * S1[s] for s in range(3)] for r in range(3)]
    lam, v = jacobi_py(C)
    lo = 0
    for i in (1, 2):
        if lam[i] < lam[lo]:
            lo = i
    others = [i for i in range(3) if i != lo]
    mid = others[1] if lam[others[1]] < lam[others[0]] else others[0]
    tr = lam[0] + lam[1] + lam[2]
    if not lam[mid] > 0.0:
        return None, 2
    low = max(lam[lo], 0.0)
    if not low <= float(np.float32(prm.max_curvature)) * tr:
        return None, 3
    n = [v[k][lo] for k in range(3)]
    m = 0
    for i in (1, 2):
        if abs(n[i]) > abs(n[m]):
            m = i
    if n[m] < 0.0:
        n = [-c for c in n]
    return (n[0], n[1], n[2], low / tr), 0


def normals_py(d, prm):
    cap = len(d["keys"])
    out = none_records(cap)
    counts = [0] * N_COUNTS
    keys, ci = d["keys"].tolist(), d["ci"].tolist()
    sums = [d[n].tolist() for n in ("sx", "sy", "sz")]
    for slot in range(cap):
        key = keys[slot]
        if key == V.EMPTY or (ci[slot] >> 40) < prm.min_count:
            continue
        counts[0] += 1
        k = [((key >> (21 * r)) & FIELD) - (1 << 20) for r in range(3)]
        parts = []
        for o in A.offsets(1):
            if o == (0, 0, 0):
                h = slot
            else:
                kk = [k[r] + o[r] for r in range(3)]
                if any(c < -(1 << 20) or c >= (1 << 20) for c in kk):
                    continue
                h = _find(d, A.key_of(kk))
                if h < 0 or (ci[h] >> 40) < prm.min_count:
                    continue
            parts.append((o, ci[h] >> 40, (sums[0][h], sums[1][h], sums[2][h])))
        rec, verdict = record_py(parts, prm)
        counts[1 + verdict] += 1
        if rec is not None:
            out[slot] = tuple(np.float32(c) for c in rec)
    return out, counts


def both(d, prm):
    a, ca = normals_np(d, prm)
    b, cb = normals_py(d, prm)
    assert ca == cb, (ca, cb)
    assert np.array_equal(bits(a), bits(b)), np.flatnonzero((bits(a) != bits(b)).any(axis=1))[:8]
    assert ca[0] == sum(ca[1:5]) and not any(ca[5:])
    return a, ca


# ================================================================================================ the plane form of the align
def word_of(i, k):
    """The word of j_i * j_k, i <= k: row-major over the upper triangle, from word 1."""
    return 1 + i * 6 - i * (i - 1) // 2 + (k - i)


def scale_of(i, k):
    return S40 if k < 3 else (S30 if i < 3 else S20)


def plane_sums_np(d, normals, points, m12, voxel_size, max_depth, prm, variant=None):
    m = np.asarray(m12, np.float64).reshape(3, 4)
    vs = np.float64(np.float32(voxel_size))
    nn_all = [normals[c].astype(np.float64) for c in ("nx", "ny", "nz")]
    has_all = (nn_all[0] != 0.0) | (nn_all[1] != 0.0) | (nn_all[2] != 0.0)
    table = d
    if variant == "nearest_with_normal":  # voxels without a normal are no candidates
        table = dict(d)
        table["ci"] = np.where(has_all, d["ci"], np.uint64(0))
    wa, mkeys = A.sums_np(table, points, m12, voxel_size, max_depth, prm, detail=True)
    hit = mkeys != np.uint64(V.EMPTY)
    key = mkeys[hit]
    found, slot = _lookup(d, key)
    assert found.all()
    P = [points[c][hit].astype(np.float64) for c in "xyz"]
    count = (d["ci"][slot] >> np.uint64(40)).astype(np.float64) * 65536.0
    e = []
    for r, name in enumerate(("sx", "sy", "sz")):
        w = m[r, 0] * P[0]
        w = w + m[r, 1] * P[1]
        w = w + m[r, 2] * P[2]
        w = w + m[r, 3]
        k = ((key >> np.uint64(21 * r)) & np.uint64(FIELD)).astype(np.int64) - (1 << 20)
        mu = d[name][slot].astype(np.float64) / count
        mu = k.astype(np.float64) + mu
        mu = mu * vs
        e.append(w - mu)
    has = has_all[slot]
    nn = [c[slot][has] for c in nn_all]
    e = [c[has] for c in e]
    P = [c[has] for c in P]
    a = []
    for c in range(3):
        t = m[0, c] * nn[0]
        t = t + m[1, c] * nn[1]
        t = t + m[2, c] * nn[2]
        a.append(t)
    if variant == "r_camera":  # the camera-frame residual against the world-frame normal
        cam = []
        for c in range(3):
            t = m[0, c] * e[0]
            t = t + m[1, c] * e[1]
            t = t + m[2, c] * e[2]
            cam.append(t)
        e = cam
    r = nn[0] * e[0]
    r = r + nn[1] * e[1]
    r = r + nn[2] * e[2]
    b = []
    for i, j in ((1, 2), (2, 0), (0, 1)):
        x, y = P[i] * a[j], P[j] * a[i]
        b.append(y - x if variant == "cross_sign" else x - y)
    j6 = a + b
    Q = lambda t, S: int(np.add.reduce(np.floor(t * S + 0.5).astype(np.int64)))
    W = [0] * PLANE_WORDS
    W[0] = W[29] = int(has.sum())
    for i in range(6):
        for k in range(i, 6):
            W[word_of(i, k)] = Q(j6[i] * j6[k], S30 if variant == "one_scale" else scale_of(i, k))
    for i in range(3):
        W[22 + i] = Q(a[i] * r, S36)
        W[25 + i] = Q(b[i] * r, S28)
    W[28] = Q(r * r, S28)
    W[30:34] = [wa[18], wa[19], wa[20], int((~has).sum())]
    return W


def plane_sums_py(d, normals, points, m12, voxel_size, max_depth, prm):
    m = [float(v) for v in np.asarray(m12, np.float64).reshape(12)]
    vs = float(np.float32(voxel_size))
    md = float(np.float32(max_depth))
    D2 = float(np.float32(prm.max_dist)) * float(np.float32(prm.max_dist))
    offs = A.offsets(prm.reach)
    nrm = [normals[c].tolist() for c in ("nx", "ny", "nz")]
    W = [0] * PLANE_WORDS
    Q = lambda t, S: math.floor(t * S + 0.5)
    for px, py, pz, _tag in points.tolist():
        P = (px, py, pz)
        if not (pz > 0.0) or (md > 0.0 and pz > md) or not (abs(px) < 1024.0 and abs(py) < 1024.0 and abs(pz) < 1024.0):
            W[30] += 1
            continue
        w, k = [], []
        for r in range(3):
            t = m[4 * r] * px
            t = t + m[4 * r + 1] * py
            t = t + m[4 * r + 2] * pz
            t = t + m[4 * r + 3]
            q = t / vs
            if not (q >= -A.LIMIT and q < A.LIMIT):
                break
            w.append(t)
            k.append(math.floor(q))
        if len(k) < 3:
            W[30] += 1
            continue
        best = None  # (d2, key, e, slot)
        for o in offs:
            kk = (k[0] + o[0], k[1] + o[1], k[2] + o[2])
            key = A.key_of(kk)
            h = _find(d, key)
            if h < 0:
                continue
            count = int(d["ci"][h]) >> 40
            if count < prm.min_count:
                continue
            e = [w[r] - (float(kk[r]) + float(int(d[name][h])) / (float(count) * 65536.0)) * vs for r, name in enumerate(("sx", "sy", "sz"))]
            d2 = e[0] * e[0] + e[1] * e[1] + e[2] * e[2]
            if best is None or d2 < best[0] or (d2 == best[0] and key < best[1]):
                best = (d2, key, e, h)
        if best is None:
            W[31] += 1
            continue
        if best[0] > D2:
            W[32] += 1
            continue
        e, h = best[2], best[3]
        nn = (nrm[0][h], nrm[1][h], nrm[2][h])
        if nn[0] == 0.0 and nn[1] == 0.0 and nn[2] == 0.0:
            W[33] += 1
            continue
        r = nn[0] * e[0] + nn[1] * e[1] + nn[2] * e[2]
        a = [m[c] * nn[0] + m[4 + c] * nn[1] + m[8 + c] * nn[2] for c in range(3)]
        b = [P[1] * a[2] - P[2] * a[1], P[2] * a[0] - P[0] * a[2], P[0] * a[1] - P[1] * a[0]]
        j6 = a + b
        W[0] += 1
        W[29] += 1
        for i in range(6):
            for kq in range(i, 6):
                W[word_of(i, kq)] += Q(j6[i] * j6[kq], scale_of(i, kq))
        for i in range(3):
            W[22 + i] += Q(a[i] * r, S36)
            W[25 + i] += Q(b[i] * r, S28)
        W[28] += Q(r * r, S28)
    return W


def plane_both(d, normals, points, m12, voxel_size, max_depth, prm):
    a = plane_sums_np(d, normals, points, m12, voxel_size, max_depth, prm)
    b = plane_sums_py(d, normals, points, m12, voxel_size, max_depth, prm)
    assert a == b, (a, b)
    assert sum(a[29:34]) == len(points) and a[0] == a[29] and not any(a[34:])
    return a


def plane_normal(w):
    H = [[0.0] * 6 for _ in range(6)]
    for i in range(6):
        for k in range(i, 6):
            H[i][k] = H[k][i] = float(w[word_of(i, k)]) / scale_of(i, k)
    g = [float(w[22 + i]) / S36 for i in range(3)] + [float(w[25 + i]) / S28 for i in range(3)]
    return H, g


def plane_loop(pose7_in, prm, sums_at):
    """voxel_align_ref.loop with the plane form's words: (pose7_out, the result, the trace of (m12, the 40 words))."""
    u, T = A.from_pose7(pose7_in)
    et = float(np.float32(prm.eps_t)) * float(np.float32(prm.eps_t))
    er = float(np.float32(prm.eps_r)) * float(np.float32(prm.eps_r))
    res = {"status": "MAX_ITERS", "iterations": 0, "first_matched": 0, "last_matched": 0, "first_cost": 0, "last_cost": 0, "xi": [0.0] * 6}
    trace, steps = [], 0
    for it in range(prm.max_iters):
        R, m12 = A.matrix(u, T)
        w = sums_at(m12)
        trace.append((m12, w))
        res["iterations"] = it + 1
        res["last_matched"], res["last_cost"] = w[29], w[28]
        if it == 0:
            res["first_matched"], res["first_cost"] = w[29], w[28]
        if w[29] < prm.min_matches:
            res["status"] = "TOO_FEW"
            break
        xi = A.solve(*plane_normal(w))
        if xi is None:
            res["status"] = "DEGENERATE"
            break
        u, T = A.update(u, T, R, xi)
        steps += 1
        res["xi"] = xi
        if xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2] < et and xi[3] * xi[3] + xi[4] * xi[4] + xi[5] * xi[5] < er:
            res["status"] = "CONVERGED"
            break
    out = A.to_pose7(u, T) if steps else [float(v) for v in pose7_in]
    return out, res, trace


# ================================================================================================ the corner scene
CORNER_PLANES = (((0.0, 1.0, 0.05), 0.9), ((-0.35, 0.0, 1.0), 5.0), ((1.0, 0.0, 0.45), 2.6))  # floor, back wall, side wall: n . X = d


def corner_scene(width=160, height=80, seed=10):
    """Three planes that meet in a corner, through voxel_ref.scene's ideal pinhole pair: the depth of a pixel is the nearest positive
    intersection of its ray ((u - cx) / f, (v - cy) / f, 1) with the planes; disparity in sixteenths with 0..3 sixteenths of noise,
    f32 triangulation, a tag with a random intensity.  No holes."""
    rng = np.random.default_rng(seed)
    f, b, cx, cy = 120.0, 0.5, width / 2.0, height / 2.0
    u, v = np.meshgrid(np.arange(width), np.arange(height))
    rx, ry = (u - cx) / f, (v - cy) / f
    depth = np.full(u.shape, np.inf)
    for (nx, ny, nz), dd in CORNER_PLANES:
        with np.errstate(all="ignore"):
            t = dd / (nx * rx + ny * ry + nz)
        depth = np.where((t > 0) & (t < depth), t, depth)
    assert np.isfinite(depth).all()
    d16 = np.floor(16.0 * f * b / depth) + rng.integers(0, 4, size=depth.shape)
    dsp = (d16 / 16.0).astype(np.float32)
    z = (np.float32(f * b) / dsp).astype(np.float32)
    x = ((u - cx).astype(np.float32) * z / np.float32(f)).astype(np.float32)
    y = ((v - cy).astype(np.float32) * z / np.float32(f)).astype(np.float32)
    inten = rng.integers(0, 256, size=depth.shape).astype(np.uint32)
    tag = (v * width + u).astype(np.uint32) | (inten << np.uint32(24))
    return V.records(x.ravel(), y.ravel(), z.ravel(), tag.ravel())
