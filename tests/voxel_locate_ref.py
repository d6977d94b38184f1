"""The voxel map locate (include/svo.h, "Voxel map locate") restated without a GPU, by two routes that share no code:

  (a) numpy: the volume as a dense array of cells, padded by the box; the cloud as its distinct cells with multiplicities; the
      scores as sums over slices of the padded volume shifted by s (occupancy_np, scores_np);
  (b) Python: a set of live voxel indices, ints and floats, record by record and shift by shift (occupancy_py, scores_py); for the
      small scenes only, it costs n * K * |box| set look-ups.

Both work on the download of a table (a dict of the five arrays, as voxel_align_ref's).  The loop (candidates, origin, ranking,
refinement, selection) is restated once in Python floats over voxel_align_ref's steps; its refinements are voxel_align_ref.loop or
voxel_normals_ref.plane_loop, by import.  `variant` states one deliberate misreading of the contract each; every one must change a
stated scene (tests/test_voxel_locate.py)."""
import math
from collections import namedtuple

import numpy as np

import voxel_align_ref as A
import voxel_ref as V

BEST = np.dtype([("hits_max", np.uint32), ("s0", np.int32), ("s1", np.int32), ("s2", np.int32), ("n_used", np.uint32),
                 ("n_inside", np.uint32), ("index", np.uint32), ("zero", np.uint32)])
STATUS = ("FOUND", "UNREFINED", "NO_CANDIDATE")
LIMIT = 1048560.0
LO, HI = -(1 << 20), 1 << 20
FIELD = 0x1FFFFF
Params = namedtuple("Params", "min_count up_axis n_turn turn_step box dims n_refine min_hits")
VARIANTS = ("tie_largest", "j_minus_s", "axis_order", "count_gt", "bit_63", "outside_hits", "camera_side")


def default_params(**over):
    return Params(1, 1, 4, float(np.float32(0.04)), (8, 4, 8), (512, 128, 512), 3, 64)._replace(**over)


def occupancy_words(dims):
    return dims[0] // 64 * dims[1] * dims[2]


def workspace_bytes(prm):
    r = lambda b: (b + 255) & ~255
    K = 2 * prm.n_turn + 1
    S = [2 * b + 1 for b in prm.box]
    return r(8 * occupancy_words(prm.dims)) + 256 + r(4 * K * S[0] * S[1] * S[2]) + r(32 * K)


def bits_of(cells, dims):
    """The volume's words with the bits of `cells` (j triples inside the volume) set."""
    w = [0] * occupancy_words(dims)
    for j in cells:
        assert all(0 <= j[r] < dims[r] for r in range(3)), j
        B = j[0] + dims[0] * (j[1] + dims[1] * j[2])
        w[B >> 6] |= 1 << (B & 63)
    return np.array(w, np.uint64)


# ------------------------------------------------------------------------------------------------ route (a): numpy
def occupancy_np(d, origin, dims, min_count, variant=None):
    """(the volume's uint64 words, [n_inside, n_outside])."""
    keys, count = d["keys"], d["ci"] >> np.uint64(40)
    q = (keys != np.uint64(V.EMPTY)) & ((count > np.uint64(min_count)) if variant == "count_gt" else (count >= np.uint64(min_count)))
    k = keys[q]
    j = [((k >> np.uint64(21 * r)) & np.uint64(FIELD)).astype(np.int64) - (1 << 20) - int(origin[r]) for r in range(3)]
    inside = np.ones(len(k), bool)
    for r in range(3):
        inside &= (j[r] >= 0) & (j[r] < dims[r])
    B = (j[0] + dims[0] * (j[1] + dims[1] * j[2]))[inside]
    flat = np.zeros(dims[0] * dims[1] * dims[2], np.uint8)
    flat[(B ^ 63) if variant == "bit_63" else B] = 1
    words = np.packbits(flat, bitorder="little").view(np.uint64)
    return words, [int(inside.sum()), int(len(k) - inside.sum())]


def _cells_np(points, m12, voxel_size, max_depth):
    """(the number of records that are not rejected, their (n_used, 3) int64 voxel indices)."""
    m = np.asarray(m12, np.float64).reshape(3, 4)
    vs = np.float64(np.float32(voxel_size))
    md = np.float32(max_depth)
    with np.errstate(all="ignore"):
        ok = points["z"] > np.float32(0)
        if md > 0:
            ok &= ~(points["z"] > md)
        for c in "xyz":
            ok &= np.abs(points[c]) < np.float32(1024)
        P = [points[c].astype(np.float64) for c in "xyz"]
        q = []
        for r in range(3):
            w = m[r, 0] * P[0]
            w = w + m[r, 1] * P[1]
            w = w + m[r, 2] * P[2]
            w = w + m[r, 3]
            qr = w / vs
            ok &= (qr >= -LIMIT) & (qr < LIMIT)
            q.append(qr)
        k = np.stack([np.floor(a[ok]).astype(np.int64) for a in q], axis=1) if ok.any() else np.zeros((0, 3), np.int64)
    return int(ok.sum()), k


def best_of(hits, n_used, n_inside, box, variant=None):
    """One BEST record from one candidate's scores (a flat array in the contract's order)."""
    S = [2 * b + 1 for b in box]
    h = np.asarray(hits, np.int64)
    top = int(h.max())
    at = np.flatnonzero(h == top)
    index = int(at[-1] if variant == "tie_largest" else at[0])
    return (top, index % S[0] - box[0], index // S[0] % S[1] - box[1], index // (S[0] * S[1]) - box[2], n_used, n_inside, index, 0)


def scores_np(words, origin, dims, points, mats, box, voxel_size, max_depth, variant=None):
    """(hits: (K, S2 * S1 * S0) uint32 in the contract's order, best: K BEST records)."""
    d0, d1, d2 = dims
    r0, r1, r2 = box
    S0, S1, S2 = 2 * r0 + 1, 2 * r1 + 1, 2 * r2 + 1
    occ = np.unpackbits(np.asarray(words, np.uint64).view(np.uint8), bitorder="little").reshape(d2, d1, d0)
    pad = np.full((d2 + 4 * r2, d1 + 4 * r1, d0 + 4 * r0), 1 if variant == "outside_hits" else 0, np.uint8)  # a cell c sits at c + 2 r
    pad[2 * r2:2 * r2 + d2, 2 * r1:2 * r1 + d1, 2 * r0:2 * r0 + d0] = occ
    D1, D0 = pad.shape[1], pad.shape[2]
    flat = pad.reshape(-1)
    mats = np.asarray(mats, np.float64).reshape(-1, 12)
    hits = np.zeros((len(mats), S2 * S1 * S0), np.int64)
    best = np.zeros(len(mats), BEST)
    for k, m in enumerate(mats):
        n_used, cells = _cells_np(points, m, voxel_size, max_depth)
        j = cells - np.asarray(origin, np.int64)[None, :]
        inside = ((j >= 0) & (j < np.array(dims)[None, :])).all(axis=1)
        reach = ((j + np.array(box)[None, :] >= 0) & (j - np.array(box)[None, :] < np.array(dims)[None, :])).all(axis=1)  # else no shift hits
        u, mult = np.unique(j[reach], axis=0, return_counts=True)
        h = np.zeros((S2, S1, S0), np.int64)
        if len(u):
            # the slice of the padded volume under shift s, taken at the cloud's distinct cells: cell j + s sits at j + s + 2 r
            base = ((u[:, 2] + 2 * r2) * D1 + (u[:, 1] + 2 * r1)) * D0 + (u[:, 0] + 2 * r0)
            along = (np.arange(S0) - r0)[None, :]
            for i2 in range(S2):
                for i1 in range(S1):
                    at = base[:, None] + (((i2 - r2) * D1 + (i1 - r1)) * D0 + along)
                    h[i2, i1] = mult @ flat[at].astype(np.int64)
        if variant == "j_minus_s":
            h = h[::-1, ::-1, ::-1]
        hits[k] = (h.transpose(2, 1, 0) if variant == "axis_order" else h).reshape(-1)
        best[k] = best_of(hits[k], n_used, int(inside.sum()), box, variant)
    return hits.astype(np.uint32), best


# ------------------------------------------------------------------------------------------------ route (b): Python
def live_py(d, min_count):
    """The set of the live voxels' index triples: every slot of the table, as the occupancy launch walks it."""
    out = set()
    for key, ci in zip(d["keys"].tolist(), d["ci"].tolist()):
        if key != V.EMPTY and (ci >> 40) >= min_count:
            out.add(tuple(((key >> (21 * r)) & FIELD) - (1 << 20) for r in range(3)))
    return out


def occupancy_py(d, origin, dims, min_count):
    live = live_py(d, min_count)
    inside = [tuple(i[r] - origin[r] for r in range(3)) for i in live]
    inside = [j for j in inside if all(0 <= j[r] < dims[r] for r in range(3))]
    return bits_of(inside, dims), [len(inside), len(live) - len(inside)]


def live_of_words(words, origin, dims):
    """The set of voxel index triples whose bit is set: the py route's view of a volume given as words."""
    out = set()
    for wi, w in enumerate(np.asarray(words, np.uint64).tolist()):
        while w:
            b = (w & -w).bit_length() - 1
            w &= w - 1
            B = wi * 64 + b
            out.add((B % dims[0] + origin[0], B // dims[0] % dims[1] + origin[1], B // (dims[0] * dims[1]) + origin[2]))
    return out


def scores_py(live, origin, dims, points, mats, box, voxel_size, max_depth):
    """As scores_np, from the set of live voxel index triples."""
    vs, md = float(np.float32(voxel_size)), float(np.float32(max_depth))
    S = [2 * b + 1 for b in box]
    mats = np.asarray(mats, np.float64).reshape(-1, 12)
    hits = np.zeros((len(mats), S[0] * S[1] * S[2]), np.uint32)
    best = np.zeros(len(mats), BEST)
    for k, mk in enumerate(mats):
        m = [float(v) for v in mk]
        h = [0] * (S[0] * S[1] * S[2])
        n_used = n_inside = 0
        for px, py, pz, _tag in points.tolist():
            if not (pz > 0.0) or (md > 0.0 and pz > md) or not (abs(px) < 1024.0 and abs(py) < 1024.0 and abs(pz) < 1024.0):
                continue
            j = []
            for r in range(3):
                t = m[4 * r] * px
                t = t + m[4 * r + 1] * py
                t = t + m[4 * r + 2] * pz
                t = t + m[4 * r + 3]
                q = t / vs
                if not (q >= -LIMIT and q < LIMIT):
                    break
                j.append(math.floor(q) - origin[r])
            if len(j) < 3:
                continue
            n_used += 1
            n_inside += all(0 <= j[r] < dims[r] for r in range(3))
            for s2 in range(-box[2], box[2] + 1):
                for s1 in range(-box[1], box[1] + 1):
                    for s0 in range(-box[0], box[0] + 1):
                        c = (j[0] + s0, j[1] + s1, j[2] + s2)
                        if all(0 <= c[r] < dims[r] for r in range(3)) and (c[0] + origin[0], c[1] + origin[1], c[2] + origin[2]) in live:
                            h[(s2 + box[2]) * S[1] * S[0] + (s1 + box[1]) * S[0] + (s0 + box[0])] += 1
        top = max(h)
        index = h.index(top)
        hits[k] = h
        best[k] = (top, index % S[0] - box[0], index // S[0] % S[1] - box[1], index // (S[0] * S[1]) - box[2], n_used, n_inside, index, 0)
    return hits, best


def both(words, origin, dims, points, mats, box, voxel_size, max_depth):
    a = scores_np(words, origin, dims, points, mats, box, voxel_size, max_depth)
    b = scores_py(live_of_words(words, origin, dims), origin, dims, points, mats, box, voxel_size, max_depth)
    assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes(), (a, b)
    return a


# ------------------------------------------------------------------------------------------------ the loop, once, in Python floats
def turn(u, axis, b, variant=None):
    nrm = math.sqrt(1.0 + b * b)
    a = [1.0 / nrm, 0.0, 0.0, 0.0]
    a[1 + axis] = b / nrm
    p, q = (u, a) if variant == "camera_side" else (a, u)
    w = p[0] * q[0] - p[1] * q[1] - p[2] * q[2] - p[3] * q[3]
    x = p[0] * q[1] + p[1] * q[0] + p[2] * q[3] - p[3] * q[2]
    y = p[0] * q[2] - p[1] * q[3] + p[2] * q[0] + p[3] * q[1]
    z = p[0] * q[3] + p[1] * q[2] - p[2] * q[1] + p[3] * q[0]
    s = math.sqrt(w * w + x * x + y * y + z * z)
    c = [w / s, x / s, y / s, z / s]
    h = (1.0 - (c[0] * c[0] + c[1] * c[1] + c[2] * c[2] + c[3] * c[3])) / 2.0
    return [v + v * h for v in c]


def candidates(pose7_in, prm, variant=None):
    """(T, [u_k], [m_k as 12 floats]) of the 2 n_turn + 1 candidates."""
    u, T = A.from_pose7(pose7_in)
    ts = float(np.float32(prm.turn_step))
    us = [turn(u, prm.up_axis, (float(k - prm.n_turn) * ts) / 2.0, variant) for k in range(2 * prm.n_turn + 1)]
    return T, us, [A.matrix(uk, T)[1] for uk in us]


def origin_of(T, voxel_size, dims):
    """The volume's origin, or None where the call is refused."""
    vs = float(np.float32(voxel_size))
    out = []
    for r in range(3):
        f = math.floor(T[r] / vs) if math.isfinite(T[r] / vs) else None
        if f is None or not (-2097152 <= f <= 2097152):
            return None
        o = f - dims[r] // 2
        if not (o >= LO and o + dims[r] <= HI):
            return None
        out.append(o)
    return out


def rank(best, min_hits):
    return sorted((k for k in range(len(best)) if int(best["hits_max"][k]) >= min_hits), key=lambda k: (-int(best["hits_max"][k]), k))


ZERO_ALIGN = {"status": "CONVERGED", "iterations": 0, "first_matched": 0, "last_matched": 0, "first_cost": 0, "last_cost": 0, "xi": [0.0] * 6}


def loop(pose7_in, prm, voxel_size, scores_at, refine, variant=None):
    """(pose7_out as 7 floats, the result as a dict, the trace: (origin, the matrices, best, [(coarse pose7, refined pose7, align
    result) per refinement])).  scores_at(origin, mats) gives the K BEST records; refine(pose7) gives (pose7_out, align result)."""
    vs = float(np.float32(voxel_size))
    T, us, mats = candidates(pose7_in, prm, variant)
    origin = origin_of(T, voxel_size, prm.dims)
    assert origin is not None
    best = scores_at(origin, mats)
    order = rank(best, prm.min_hits)
    pose7_in = [float(v) for v in pose7_in]
    if not order:
        return pose7_in, {"status": "NO_CANDIDATE", "k": -1, "shift": (0, 0, 0), "hits": 0, "rank": -1, "n_refined": 0, "coarse_pose7": pose7_in,
                          "align": dict(ZERO_ALIGN)}, (origin, mats, best, [])
    runs = []
    for k in order[:prm.n_refine]:
        s = (int(best["s0"][k]), int(best["s1"][k]), int(best["s2"][k]))
        coarse = A.to_pose7(us[k], [T[r] + float(s[r]) * vs for r in range(3)])
        fine, res = refine(coarse)
        runs.append((coarse, fine, res))
    chosen = None
    for i, (_, _, res) in enumerate(runs):
        if res["status"] in ("CONVERGED", "MAX_ITERS"):
            top = None if chosen is None else runs[chosen][2]
            if top is None or res["last_matched"] > top["last_matched"] or (res["last_matched"] == top["last_matched"] and res["last_cost"] < top["last_cost"]):
                chosen = i
    status = "FOUND" if chosen is not None else "UNREFINED"
    chosen = 0 if chosen is None else chosen
    k = order[chosen]
    out = runs[chosen][1] if status == "FOUND" else runs[chosen][0]
    return out, {"status": status, "k": k, "shift": (int(best["s0"][k]), int(best["s1"][k]), int(best["s2"][k])), "hits": int(best["hits_max"][k]),
                 "rank": chosen, "n_refined": len(runs), "coarse_pose7": runs[chosen][0], "align": runs[chosen][2]}, (origin, mats, best, runs)


def start_pose(truth7, shift, ang):
    """The corner scene's start: u0 = normalise((1, 0, tan(-ang / 2), 0)) (x) u_TRUTH, T0 = T + shift (an input, at whatever rounding)."""
    u, T = A.from_pose7(truth7)
    return A.to_pose7(turn(u, 1, math.tan(-ang / 2.0)), [T[r] + shift[r] for r in range(3)])
