"""The voxel map align's contract (include/svo.h, "Voxel map align") restated by two routes that share no code:

  sums_np   whole arrays in numpy: f64 arithmetic one operation per ufunc (numpy never contracts), the 27 candidates as an (n, 27)
            key array looked up in a sorted key list built from the table (a slot counts only if it sits fewer than 64 slots
            behind its key's home), the words summed with np.add.reduce on int64;
  sums_py   record by record in Python floats and ints; every candidate is probed through the raw table slot by slot.

Both take the table in the download's form, a dict of uint64 arrays "keys", "ci", "sx", "sy", "sz" of 2^log2 entries (place() makes one
from a voxel_ref.Table without a GPU), and return the 32 words as a list of Python ints.  `variant` of sums_np states one deliberate
misreading of the contract each.  loop() restates the host loop once, in plain Python floats.  Nothing here is tuned on the library's
output.
"""
import math
from collections import namedtuple

import numpy as np

import voxel_ref as V

WORDS = 32
LIMIT = 1048575.0
S16, S28 = 65536.0, 268435456.0
MAX_POINTS = 1 << 20
STATUS = ("CONVERGED", "MAX_ITERS", "TOO_FEW", "DEGENERATE")
COUNTS = ("n_matched", "n_rejected", "n_unmatched", "n_far")
VARIANTS = ("reach0", "first_found", "tie_largest_key", "count_gt", "floor_no_half", "e_world", "cross_sign", "far_ge")
Params = namedtuple("Params", "min_count reach max_dist max_iters min_matches eps_t eps_r")


def default_params(voxel_size, **over):
    vs = np.float32(voxel_size)
    p = Params(1, 1, float(min(np.float32(2) * vs, np.float32(8))), 10, 64, float(vs / np.float32(100)), float(np.float32(1e-5)))
    return p._replace(**over)


def offsets(reach):
    """Candidate c of 27 is k + (c % 3 - 1, c // 3 % 3 - 1, c // 9 - 1); reach 0 has the one candidate k."""
    if reach == 0:
        return [(0, 0, 0)]
    return [(c % 3 - 1, c // 3 % 3 - 1, c // 9 - 1) for c in range(27)]


def key_of(k):
    return (k[0] + (1 << 20)) | (k[1] + (1 << 20)) << 21 | (k[2] + (1 << 20)) << 42


def place(table, log2, order=None):
    """The download of a 2^log2 table that received the voxels of a voxel_ref.Table one after the other (in `order`, a permutation
    of its rows; None: ascending keys) by the insert's linear probing."""
    cap = 1 << log2
    d = {"keys": np.full(cap, V.EMPTY, np.uint64)}
    for n in ("ci", "sx", "sy", "sz"):
        d[n] = np.zeros(cap, np.uint64)
    rows = range(len(table.keys)) if order is None else order
    for i in rows:
        k = int(table.keys[i])
        h = V.fmix64(k) & (cap - 1)
        for _ in range(V.MAX_PROBES):
            if int(d["keys"][h]) == V.EMPTY:
                break
            h = (h + 1) & (cap - 1)
        else:
            raise AssertionError("place: the table drops a voxel")
        d["keys"][h] = k
        for n in ("ci", "sx", "sy", "sz"):
            d[n][h] = getattr(table, n)[i]
    return d


# ------------------------------------------------------------------------------------------------ route (a): numpy
def _reachable(d):
    """The slots a look-up can reach, sorted by key: occupied and fewer than 64 slots behind the key's home."""
    cap = len(d["keys"])
    at = np.flatnonzero(d["keys"] != np.uint64(V.EMPTY))
    home = np.array([V.fmix64(k) & (cap - 1) for k in d["keys"][at].tolist()], np.int64)
    at = at[((at - home) & (cap - 1)) < V.MAX_PROBES]
    return at[np.argsort(d["keys"][at])]


def _q(x, S, variant):
    return np.floor(x * S if variant == "floor_no_half" else x * S + 0.5).astype(np.int64)


def sums_np(d, points, m12, voxel_size, max_depth, prm, variant=None, detail=False):
    m = np.asarray(m12, np.float64).reshape(3, 4)
    vs = np.float64(np.float32(voxel_size))
    md = np.float32(max_depth)
    n = len(points)
    lim = np.float32(1024)
    with np.errstate(all="ignore"):
        z32 = points["z"]
        ok = z32 > np.float32(0)
        if md > 0:
            ok &= ~(z32 > md)
        for c in "xyz":
            ok &= np.abs(points[c]) < lim
        P = [points[c].astype(np.float64) for c in "xyz"]
        w, q = [], []
        for r in range(3):
            wr = m[r, 0] * P[0]
            wr = wr + m[r, 1] * P[1]
            wr = wr + m[r, 2] * P[2]
            wr = wr + m[r, 3]
            qr = wr / vs
            ok &= (qr >= -LIMIT) & (qr < LIMIT)
            w.append(wr)
            q.append(qr)
    n_rejected = n - int(ok.sum())
    P = [a[ok] for a in P]
    w = [a[ok] for a in w]
    k = [np.floor(a[ok]) for a in q]
    off = np.array(offsets(0 if variant == "reach0" else prm.reach), np.int64)  # (nc, 3)
    kc = [k[r][:, None] + off[None, :, r].astype(np.float64) for r in range(3)]  # (n, nc) f64, exact
    key = np.zeros(kc[0].shape, np.uint64)
    for r in range(3):
        key |= (kc[r].astype(np.int64) + (1 << 20)).astype(np.uint64) << np.uint64(21 * r)
    at = _reachable(d)
    tk = d["keys"][at]
    pos = np.minimum(np.searchsorted(tk, key), max(len(tk) - 1, 0))
    found = (tk[pos] == key) if len(tk) else np.zeros(key.shape, bool)
    slot = at[pos] if len(tk) else np.zeros(key.shape, np.int64)
    count = np.where(found, d["ci"][slot] >> np.uint64(40), np.uint64(0))
    qual = found & ((count > np.uint64(prm.min_count)) if variant == "count_gt" else (count >= np.uint64(prm.min_count)))
    cf = np.where(qual, count, np.uint64(1)).astype(np.float64) * 65536.0
    e = []
    for r, name in enumerate(("sx", "sy", "sz")):
        mu = d[name][slot].astype(np.float64) / cf
        mu = kc[r] + mu
        mu = mu * vs
        e.append(w[r][:, None] - mu)
    d2 = e[0] * e[0]
    d2 = d2 + e[1] * e[1]
    d2 = d2 + e[2] * e[2]
    d2 = np.where(qual, d2, np.inf)
    has = qual.any(axis=1)
    if variant == "first_found":
        best = np.argmax(qual, axis=1)
    else:
        tie = qual & (d2 == d2.min(axis=1)[:, None])
        if variant == "tie_largest_key":
            best = np.argmax(np.where(tie, key, np.uint64(0)), axis=1)
        else:
            best = np.argmin(np.where(tie, key, np.uint64(V.EMPTY)), axis=1)
    rows = np.arange(len(best))
    bd2 = d2[rows, best]
    D2 = np.float64(np.float32(prm.max_dist)) * np.float64(np.float32(prm.max_dist))
    far = has & ((bd2 >= D2) if variant == "far_ge" else (bd2 > D2))
    hit = has & ~far
    eb = [a[rows, best][hit] for a in e]
    Pm = [a[hit] for a in P]
    c = []
    for r in range(3):
        if variant == "e_world":
            c.append(eb[r])
            continue
        cr = m[0, r] * eb[0]
        cr = cr + m[1, r] * eb[1]
        cr = cr + m[2, r] * eb[2]
        c.append(cr)
    terms = [(Pm[0], S16), (Pm[1], S16), (Pm[2], S16)]
    terms += [(Pm[i] * Pm[j], S16) for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    terms += [(c[0], S28), (c[1], S28), (c[2], S28)]
    for i, j in ((1, 2), (2, 0), (0, 1)):
        a, b = Pm[i] * c[j], Pm[j] * c[i]
        terms.append((b - a if variant == "cross_sign" else a - b, S28))
    cost = c[0] * c[0]
    cost = cost + c[1] * c[1]
    cost = cost + c[2] * c[2]
    terms.append((cost, S28))
    n_matched = int(hit.sum())
    words = [n_matched] + [int(np.add.reduce(_q(t, S, variant))) for t, S in terms]
    words += [n_matched, n_rejected, int((~has).sum()), int(far.sum())]
    words += [0] * (WORDS - len(words))
    if detail:
        full = np.full(n, V.EMPTY, np.uint64)
        full[np.flatnonzero(ok)[hit]] = key[rows, best][hit]
        return words, full
    return words


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


def sums_py(d, points, m12, voxel_size, max_depth, prm, detail=False):
    m = [float(v) for v in np.asarray(m12, np.float64).reshape(12)]
    vs = float(np.float32(voxel_size))
    md = float(np.float32(max_depth))
    D2 = float(np.float32(prm.max_dist)) * float(np.float32(prm.max_dist))
    offs = offsets(prm.reach)
    W = [0] * WORDS
    matched_keys = []
    for px, py, pz, _tag in points.tolist():
        matched_keys.append(V.EMPTY)
        P = (px, py, pz)
        if not (pz > 0.0) or (md > 0.0 and pz > md) or not (abs(px) < 1024.0 and abs(py) < 1024.0 and abs(pz) < 1024.0):
            W[18] += 1
            continue
        w, k, good = [], [], True
        for r in range(3):
            t = m[4 * r] * px
            t = t + m[4 * r + 1] * py
            t = t + m[4 * r + 2] * pz
            t = t + m[4 * r + 3]
            q = t / vs
            if not (q >= -LIMIT and q < LIMIT):
                good = False
                break
            w.append(t)
            k.append(math.floor(q))
        if not good:
            W[18] += 1
            continue
        best = None  # (d2, key, e)
        for o in offs:
            kk = (k[0] + o[0], k[1] + o[1], k[2] + o[2])
            key = key_of(kk)
            h = _find(d, key)
            if h < 0:
                continue
            ci = int(d["ci"][h])
            count = ci >> 40
            if count < prm.min_count:
                continue
            e = []
            for r, name in enumerate(("sx", "sy", "sz")):
                mu = (float(kk[r]) + float(int(d[name][h])) / (float(count) * 65536.0)) * vs
                e.append(w[r] - mu)
            d2 = e[0] * e[0] + e[1] * e[1] + e[2] * e[2]
            if best is None or d2 < best[0] or (d2 == best[0] and key < best[1]):
                best = (d2, key, e)
        if best is None:
            W[19] += 1
            continue
        if best[0] > D2:
            W[20] += 1
            continue
        e = best[2]
        c = [m[r] * e[0] + m[4 + r] * e[1] + m[8 + r] * e[2] for r in range(3)]
        Q = lambda t, S: math.floor(t * S + 0.5)
        W[0] += 1
        W[17] += 1
        for r in range(3):
            W[1 + r] += Q(P[r], S16)
            W[10 + r] += Q(c[r], S28)
        for n, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            W[4 + n] += Q(P[i] * P[j], S16)
        W[13] += Q(P[1] * c[2] - P[2] * c[1], S28)
        W[14] += Q(P[2] * c[0] - P[0] * c[2], S28)
        W[15] += Q(P[0] * c[1] - P[1] * c[0], S28)
        W[16] += Q(c[0] * c[0] + c[1] * c[1] + c[2] * c[2], S28)
        matched_keys[-1] = best[1]
    if detail:
        return W, np.array(matched_keys, np.uint64)
    return W


def both(d, points, m12, voxel_size, max_depth, prm):
    a, b = sums_np(d, points, m12, voxel_size, max_depth, prm), sums_py(d, points, m12, voxel_size, max_depth, prm)
    assert a == b, (a, b)
    assert sum(a[17:21]) == len(points) and a[0] == a[17] and not any(a[21:])
    return a


# ------------------------------------------------------------------------------------------------ the loop, once, in Python floats
def quat_to_R(q):
    w, x, y, z = q
    s = 2.0 / (w * w + x * x + y * y + z * z)
    return [1.0 - s * (y * y + z * z), s * (x * y - w * z), s * (x * z + w * y),
            s * (x * y + w * z), 1.0 - s * (x * x + z * z), s * (y * z - w * x),
            s * (x * z - w * y), s * (y * z + w * x), 1.0 - s * (x * x + y * y)]


def from_pose7(pose7):
    qw, qx, qy, qz, t0, t1, t2 = (float(v) for v in pose7)
    s = math.sqrt(qw * qw + qx * qx + qy * qy + qz * qz)
    u = [qw / s, -qx / s, -qy / s, -qz / s]
    R = quat_to_R(u)
    return u, [-(R[3 * r] * t0 + R[3 * r + 1] * t1 + R[3 * r + 2] * t2) for r in range(3)]


def matrix(u, T):
    R = quat_to_R(u)
    return R, [R[0], R[1], R[2], T[0], R[3], R[4], R[5], T[1], R[6], R[7], R[8], T[2]]


def to_pose7(u, T):
    R = quat_to_R(u)
    return [u[0], -u[1], -u[2], -u[3]] + [-(R[r] * T[0] + R[3 + r] * T[1] + R[6 + r] * T[2]) for r in range(3)]


def normal(w):
    N = float(w[0])
    A = [float(w[1 + i]) / S16 for i in range(3)]
    B = [float(w[4 + i]) / S16 for i in range(6)]
    g = [float(w[10 + i]) / S28 for i in range(6)]
    H = [[0.0] * 6 for _ in range(6)]
    H[0][0] = H[1][1] = H[2][2] = N
    H[0][4], H[0][5], H[1][3], H[1][5], H[2][3], H[2][4] = A[2], -A[1], -A[2], A[0], A[1], -A[0]
    H[3][3], H[4][4], H[5][5] = B[3] + B[5], B[0] + B[5], B[0] + B[3]
    H[3][4], H[3][5], H[4][5] = -B[1], -B[2], -B[4]
    for i in range(6):
        for j in range(i):
            H[i][j] = H[j][i]
    return H, g


def solve(H, g):
    """xi with H xi = -g by the stated Cholesky factorisation, or None at a pivot that fails d > 0 and finite."""
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        d = H[j][j]
        for k in range(j):
            d = d - L[j][k] * L[j][k]
        if not (d > 0.0 and d <= 1.7976931348623157e308):
            return None
        L[j][j] = math.sqrt(d)
        for i in range(j + 1, 6):
            s = H[i][j]
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            L[i][j] = s / L[j][j]
    y = [0.0] * 6
    for i in range(6):
        s = -g[i]
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = s / L[i][i]
    x = [0.0] * 6
    for i in range(5, -1, -1):
        s = y[i]
        for k in range(i + 1, 6):
            s = s - L[k][i] * x[k]
        x[i] = s / L[i][i]
    return x


def update(u, T, R, xi):
    T = [T[r] + (R[3 * r] * xi[0] + R[3 * r + 1] * xi[1] + R[3 * r + 2] * xi[2]) for r in range(3)]
    b0, b1, b2 = xi[3] / 2.0, xi[4] / 2.0, xi[5] / 2.0
    w = u[0] - u[1] * b0 - u[2] * b1 - u[3] * b2
    x = u[1] + u[0] * b0 + u[2] * b2 - u[3] * b1
    y = u[2] + u[0] * b1 - u[1] * b2 + u[3] * b0
    z = u[3] + u[0] * b2 + u[1] * b1 - u[2] * b0
    s = math.sqrt(w * w + x * x + y * y + z * z)
    a = [w / s, x / s, y / s, z / s]
    h = (1.0 - (a[0] * a[0] + a[1] * a[1] + a[2] * a[2] + a[3] * a[3])) / 2.0
    return [v + v * h for v in a], T


def loop(pose7_in, prm, sums_at):
    """(pose7_out as 7 floats, the result as a dict, the trace: per iteration (m12 as 12 floats, the 32 words)).  sums_at(m12) gives
    the words of one matrix."""
    u, T = from_pose7(pose7_in)
    et = float(np.float32(prm.eps_t)) * float(np.float32(prm.eps_t))
    er = float(np.float32(prm.eps_r)) * float(np.float32(prm.eps_r))
    res = {"status": "MAX_ITERS", "iterations": 0, "first_matched": 0, "last_matched": 0, "first_cost": 0, "last_cost": 0, "xi": [0.0] * 6}
    trace, steps = [], 0
    for it in range(prm.max_iters):
        R, m12 = matrix(u, T)
        w = sums_at(m12)
        trace.append((m12, w))
        res["iterations"] = it + 1
        res["last_matched"], res["last_cost"] = w[17], w[16]
        if it == 0:
            res["first_matched"], res["first_cost"] = w[17], w[16]
        if w[17] < prm.min_matches:
            res["status"] = "TOO_FEW"
            break
        xi = solve(*normal(w))
        if xi is None:
            res["status"] = "DEGENERATE"
            break
        u, T = update(u, T, R, xi)
        steps += 1
        res["xi"] = xi
        if xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2] < et and xi[3] * xi[3] + xi[4] * xi[4] + xi[5] * xi[5] < er:
            res["status"] = "CONVERGED"
            break
    out = to_pose7(u, T) if steps else [float(v) for v in pose7_in]
    return out, res, trace


# ------------------------------------------------------------------------------------------------ poses and errors
def pose_errors(pose7, truth7):
    """(translation error, rotation error in radians) between the camera->world transforms of two pose7."""
    (ua, Ta), (ub, Tb) = from_pose7(pose7), from_pose7(truth7)
    Ra, Rb = np.array(quat_to_R(ua)).reshape(3, 3), np.array(quat_to_R(ub)).reshape(3, 3)
    cosang = ((Ra @ Rb.T).trace() - 1.0) / 2.0
    return float(np.linalg.norm(np.array(Ta) - np.array(Tb))), float(math.acos(max(-1.0, min(1.0, cosang))))


def displaced(truth7, shift, rotvec):
    """truth7 with its camera->world transform moved by `shift` (map units, world frame) and turned by the small rotation vector
    `rotvec` (radians, camera frame): an input of the tests, made in numpy at whatever rounding it has."""
    u, T = from_pose7(truth7)
    b = [v / 2.0 for v in rotvec]
    dq = np.array([1.0, b[0], b[1], b[2]])
    a = np.array(u)
    w = a[0] * dq[0] - a[1] * dq[1] - a[2] * dq[2] - a[3] * dq[3]
    x = a[0] * dq[1] + a[1] * dq[0] + a[2] * dq[3] - a[3] * dq[2]
    y = a[0] * dq[2] - a[1] * dq[3] + a[2] * dq[0] + a[3] * dq[1]
    z = a[0] * dq[3] + a[1] * dq[2] - a[2] * dq[1] + a[3] * dq[0]
    un = np.array([w, x, y, z])
    un = un / np.linalg.norm(un)
    return to_pose7([float(v) for v in un], [T[r] + shift[r] for r in range(3)])
