"""Keyframe geometry by another route: the new-vs-tracked dedup (src/image_processor.cpp:113-128), the reprojection matrix and the
triangulation (:178-207) and the keyframe pose matrix (:130-134), restated in numpy on WHOLE ARRAYS from the reference's text and the
declared arithmetic of DESIGN.md section 2.  TEST INFRASTRUCTURE ONLY; imports neither the oracle nor the library.

Where the oracle and the kernels walk the lists (a loop over the tracked features with an early exit, a push_back or a ballot / prefix
compaction), this file forms one (n_det, n_trk) f32 plane per operation of :118-120 and reduces it with `any`, and selects with boolean
masks: there is no loop over features, no early exit, no slot arithmetic.  Every f32 operation is its own numpy statement on float32
arrays (numpy rounds each to f32; nothing can be contracted); every f64 accumulation is written out term by term.

`variant=` selects a deliberate MISREADING of the declared arithmetic; the variants exist only to show which inputs tell them apart
(tests/test_geom_paths.py).  The default (None) is the declared arithmetic."""
import numpy as np

F = np.float32
D = np.float64
DEDUP_VARIANTS = ("fma", "f64", "le", "squared")
TRI_VARIANTS = ("acc32", "q_first", "recip", "ge0", "div64")
VARIANTS = DEDUP_VARIANTS + TRI_VARIANTS
MIN_NORMAL = F(2.0 ** -126)


def _f32(a, cols):
    a = np.ascontiguousarray(a, dtype=F)
    return a.reshape(-1, cols) if cols else a.reshape(-1)


# ------------------------------------------------------------------------------------------------ dedup
def _hit_plane(x, y, tx, ty, min_d, variant=None):
    """x, y: (rows, 1); tx, ty: (1, n_trk) (any shapes that broadcast).  Returns the (rows, n_trk) planes of the f32 distance of
    :118-120 (None for the variants that form none) and of the decision `tracked`."""
    min_d = F(min_d)
    with np.errstate(over="ignore", invalid="ignore"):
        if variant == "f64":
            dx = x.astype(D) - tx.astype(D)
            dy = y.astype(D) - ty.astype(D)
            return None, np.sqrt(dx * dx + dy * dy) < D(min_d)
        dx = x - tx
        dy = y - ty
        yy = dy * dy
        if variant == "fma":  # one rounding for dx * dx + yy
            s = (dx.astype(D) * dx.astype(D) + yy.astype(D)).astype(F)
        else:
            xx = dx * dx
            s = xx + yy
        if variant == "squared":
            return None, s < min_d * min_d
        dist = np.sqrt(s)
        assert dist.dtype == F
        return dist, (dist <= min_d) if variant == "le" else (dist < min_d)


def dedup(det, trk, min_d, variant=None, counters=False, block=512):
    """kept detected points (n_kept, 2) in input order [, counters].  Blocks of detected rows only bound the memory."""
    det, trk = _f32(det, 2), _f32(trk, 2)
    nd, nt = len(det), len(trk)
    tracked = np.zeros(nd, bool)
    c = dict(kept=0, dropped=0, dropped_by_one=0, at_threshold=0, ulp_below=0, **{"flip_" + v: 0 for v in DEDUP_VARIANTS})
    if nt:
        m = F(min_d)
        below = np.nextafter(m, F(-np.inf))
        for r0 in range(0, nd, block):
            x, y = det[r0:r0 + block, 0:1], det[r0:r0 + block, 1:2]
            tx, ty = trk[None, :, 0], trk[None, :, 1]
            dist, hit = _hit_plane(x, y, tx, ty, min_d, variant)
            tracked[r0:r0 + block] = hit.any(axis=1)
            if counters:
                c["dropped_by_one"] += int((hit.sum(axis=1) == 1).sum())
                with np.errstate(invalid="ignore"):
                    nearest = np.fmin.reduce(dist, axis=1)
                c["at_threshold"] += int((nearest == m).sum())
                c["ulp_below"] += int((nearest == below).sum())
                for v in DEDUP_VARIANTS:
                    c["flip_" + v] += int((_hit_plane(x, y, tx, ty, min_d, v)[1] != hit).sum())
    kept = det[~tracked]
    c["kept"], c["dropped"] = int(len(kept)), int(tracked.sum())
    return (kept, c) if counters else kept


# ------------------------------------------------------------------------------------------------ matrices
def reprojection_q(focal, cx, cy, baseline):
    """The six assignments of :184-189 to a zero CV_32F matrix.  focal, cx, cy, baseline are floats (:178-180, the header's member);
    `1.0 / focal` and `1.0 / (baseline * focal)` are double expressions stored into a float, `-cx / focal` is a float expression."""
    focal, cx, cy, baseline = F(focal), F(cx), F(cy), F(baseline)
    Q = np.zeros((4, 4), F)
    Q[0, 0] = F(D(1.0) / D(focal))
    Q[1, 1] = F(D(1.0) / D(focal))
    Q[0, 3] = F(-cx) / focal
    Q[1, 3] = F(-cy) / focal
    Q[2, 3] = F(1)
    bf = baseline * focal
    assert type(bf) is F
    Q[3, 2] = F(D(1.0) / D(bf))
    return Q


def _matmul_f32(A, B):
    """cv::Mat float product: each element the k = 0..3 sum in f64 of exact f32 x f32 products, rounded once."""
    A, B = np.asarray(A, F).astype(D), np.asarray(B, F).astype(D)
    s = A[:, 0:1] * B[0:1, :]
    for k in range(1, A.shape[1]):
        s = s + A[:, k:k + 1] * B[k:k + 1, :]
    return s.astype(F)


def reprojection_matrix(pose16, focal, cx, cy, baseline):
    """M = f32(camera_pose * Q), the left product of :202."""
    return _matmul_f32(_f32(pose16, 4), reprojection_q(focal, cx, cy, baseline))


def hmat_from_R_t(R, t):
    """:130-134: hmat = [R^T | -R^T t] from the float rotation matrix and translation (float Mats; the product accumulates in double)."""
    R, t = _f32(R, 3), _f32(t, 0)
    h = np.eye(4, dtype=F)
    h[:3, :3] = R.T
    nR = (-R).astype(D)
    col = nR[0, :] * D(t[0])
    col = col + nR[1, :] * D(t[1])
    col = col + nR[2, :] * D(t[2])
    h[:3, 3] = col.astype(F)
    return h


# ------------------------------------------------------------------------------------------------ triangulation
def _rows(M, x, y, d, variant=None):
    """The four components of M [x y d 1]^T for the kept points, f32 (4, m)."""
    if variant == "acc32":
        return np.stack([((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * d) + M[r, 3] for r in range(4)])
    M, x, y, d = M.astype(D), x.astype(D), y.astype(D), d.astype(D)
    return np.stack([(((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * d) + M[r, 3]).astype(F) for r in range(4)])


def triangulate(xy, disp, pose16, focal, cx, cy, baseline, variant=None, counters=False):
    """kept_xy (m, 2), xyz (m, 3), kept_index (m,) int32 [, counters]: :191-206 for the whole list at once."""
    xy, disp = _f32(xy, 2), _f32(disp, 0)
    with np.errstate(invalid="ignore"):
        keep = (disp >= F(0)) if variant == "ge0" else (disp > F(0))
    idx = np.flatnonzero(keep).astype(np.int32)
    kept_xy = xy[keep]
    x, y, d = kept_xy[:, 0], kept_xy[:, 1], disp[keep]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        if variant == "q_first":  # camera_pose * (Q * v)
            Q = reprojection_q(focal, cx, cy, baseline)
            u = _rows(Q, x, y, d)
            P = _f32(pose16, 4).astype(D)
            u = u.astype(D)
            w = np.stack([(((P[r, 0] * u[0] + P[r, 1] * u[1]) + P[r, 2] * u[2]) + P[r, 3] * u[3]).astype(F) for r in range(4)])
        else:
            w = _rows(reprojection_matrix(pose16, focal, cx, cy, baseline), x, y, d, variant)
        assert w.dtype == F
        if variant == "recip":
            r = F(1) / w[3]
            xyz = np.stack([w[0] * r, w[1] * r, w[2] * r], axis=1)
        elif variant == "div64":
            xyz = np.stack([(w[k].astype(D) / w[3].astype(D)).astype(F) for k in range(3)], axis=1)
        else:
            xyz = np.stack([w[0] / w[3], w[1] / w[3], w[2] / w[3]], axis=1)
    assert xyz.dtype == F
    xyz = xyz.reshape(-1, 3)
    if not counters:
        return kept_xy, xyz, idx
    drop = disp[~keep]
    c = dict(kept=int(keep.sum()), dropped=int((~keep).sum()),
             dropped_minus_one=int((drop == F(-1)).sum()),
             dropped_plus_zero=int(((drop == 0) & ~np.signbit(drop)).sum()),
             dropped_minus_zero=int(((drop == 0) & np.signbit(drop)).sum()),
             dropped_nan=int(np.isnan(drop).sum()),
             kept_subnormal=int((d < MIN_NORMAL).sum()),
             kept_inf=int(np.isposinf(d).sum()))
    return kept_xy, xyz, idx, c
