"""a5 PnP-RANSAC — a plain restatement of DESIGN §5 in Python floats and numpy, independent of the oracle and of the library.

`oracle/ora_pnp.cpp` and `csrc/pnp.hip` are by one hand and share one structure, so a misreading of §5 common to both cannot show
between them.  This file states the same function again, where bit-exactness leaves room by another route — residuals,
Jacobians and the inlier test as whole-array numpy f64 operations, the per-term products as one (m, 43) table that is then summed
in the declared order, the Cholesky and the forward substitution right-looking — and keeps a counter on every decision, so that
the scenes of `tests/test_pnp_paths.py` can show which branches they reach.  The retraction, the step control and the cap are a
handful of scalar statements whose order is declared; they can only be written as declared, so a misreading of those
declarations themselves is not something this file can show.

Bit-exact by construction: Python floats and numpy elementwise f64 never contract a product into a sum, every product and sum
is written in the declared order, and no libm function other than the correctly rounded `sqrt` is used.

What is declared (`host/det_trig.h`, `host/lm_math.h`, `host/pnp_iters.h`):
  draws       splitmix64 seeded 0x5EED0A5 + h·0xD1B54A32D192ED03 (mod 2^64), index = draw mod n, five distinct, redraw on a duplicate
  residual    Xc = R(q) X + t (row sums left to right, then + t), e = (f·Xc.x)·(1/Xc.z) + c − uv; J against a left rotation
              perturbation and an additive translation
  sums        minimal solve: sequential over the five points; refinement: partial[t] = sequential over k = t, t + 256, …, then
              partial[t] += partial[t + s] for s = 128, 64, …, 1; the cost alone is summed the same way
  solve6      lower Cholesky of H + λ·diag(H) + 1e-12·I, left-looking, one product subtracted at a time in ascending k, one
              division per element, forward then backward substitution of −g; fails when a pivot is not > 0
  retraction  q⁺ = normalise(normalise([1, d/2]) ⊗ q), t⁺ = t + d[3:6]
  LM          λ = 1e-3; accepted (cost strictly smaller): λ ← max(0.1·λ, 1e-9), stop when |d|² < 1e-20 or |d|² ≤ 2⁻⁴⁶·x², x² = |t|² +
              4·|q.xyz|² of the pose BEFORE the step; rejected: λ ← 10·λ, stop when λ > 1e6; failed factorisation: λ ← 10·λ, no test
  inlier      z > 0 and e² ≤ (double)(float)err · (double)(float)err
  bookkeeping hypotheses in order, a count above max(best, 4) replaces the best, the cap is RANSACUpdateNumIters with the declared
              log / power / round-half-even, fed the current cap as max_iters
  conversions declared sincos / first-quadrant atan2; rvec → quaternion and back with their small-angle branches

`variant=` selects one deliberate misreading (VARIANTS); the tests show that each one changes the returned bytes of some scene.
"""
import math
import struct

import numpy as np

MODEL = 5
SEED, STRIDE, M64 = 0x5EED0A5, 0xD1B54A32D192ED03, (1 << 64) - 1
REL_STEP2 = 2.0 ** -46  # FLT_EPSILON², exact
DBL_MIN = 2.2250738585072014e-308
VARIANTS = ("tie_replaces", "thr_strict", "thr_f32sq", "no_z_test", "seq_sum", "min_tree", "no_jitter", "no_lam_floor", "no_cap",
            "no_abs_stop")
LM_COUNTERS = ("chol_fail", "accept", "reject", "nan_cost", "lam_floor", "exit_abs", "exit_abs_alone", "exit_rel", "exit_lambda",
               "exit_cap")
CALL_COUNTERS = ("dup_draw", "z_le_0", "tie", "quat_flip")


def _div(a, b):
    """IEEE a / b for Python floats (Python raises on a zero divisor)."""
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)


# ---------------------------------------------------------------------------------------------- declared elementary functions
def det_sincos(x):
    k = 0
    while x > 0.5:
        x *= 0.5
        k += 1
    x2 = x * x
    s = x * (1.0 + x2 * (-1.0 / 6.0 + x2 * (1.0 / 120.0 + x2 * (-1.0 / 5040.0 + x2 * (1.0 / 362880.0 + x2 * (-1.0 / 39916800.0 +
        x2 * (1.0 / 6227020800.0 + x2 * (-1.0 / 1307674368000.0))))))))
    c = 1.0 + x2 * (-0.5 + x2 * (1.0 / 24.0 + x2 * (-1.0 / 720.0 + x2 * (1.0 / 40320.0 + x2 * (-1.0 / 3628800.0 +
        x2 * (1.0 / 479001600.0 + x2 * (-1.0 / 87178291200.0)))))))
    for _ in range(k):
        s2 = 2.0 * s * c
        c = 1.0 - 2.0 * s * s
        s = s2
    return s, c


def _atan_small(z):
    w = z * z
    p = 1.0 / 47.0
    for d in range(45, 0, -2):  # 1/45 − w p, …, 1/3 − w p, 1 − w p
        p = 1.0 / d - w * p
    return z * p


def _atan01(t):
    if t > 0.41421356237309503:
        return 0.78539816339744828 + _atan_small(_div(t - 1.0, t + 1.0))
    return _atan_small(t)


def atan2_q1(y, x):
    if y <= x:
        return _atan01(_div(y, x))
    return 1.5707963267948966 - _atan01(_div(x, y))


def quat_from_rvec(rv):
    th = math.sqrt(rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2])
    if th < 1e-12:
        return [1.0, 0.5 * rv[0], 0.5 * rv[1], 0.5 * rv[2]]
    s, c = det_sincos(0.5 * th)
    sn = s / th
    return [c, sn * rv[0], sn * rv[1], sn * rv[2]]


def rvec_from_quat(q, rec=None):
    q = list(q)
    if q[0] < 0:
        q = [-v for v in q]
        if rec is not None:
            rec["quat_flip"] += 1
    vn = math.sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    if vn < 1e-12:
        return [2 * q[1], 2 * q[2], 2 * q[3]]
    th = 2.0 * atan2_q1(vn, q[0])
    return [_div(q[1], vn) * th, _div(q[2], vn) * th, _div(q[3], vn) * th]


def rvec_quat_roundtrip(rv):
    q = quat_from_rvec([float(v) for v in rv])
    return np.array(q), np.array(rvec_from_quat(q))


def det_log(x):
    bits = struct.unpack("<Q", struct.pack("<d", x))[0]
    e = ((bits >> 52) & 0x7FF) - 1022
    m = struct.unpack("<d", struct.pack("<Q", (bits & 0x000FFFFFFFFFFFFF) | 0x3FE0000000000000))[0]  # in [0.5, 1)
    if m < 0.70710678118654757:
        m, e = m * 2.0, e - 1
    s = (m - 1.0) / (m + 1.0)
    z = s * s
    p = 1.0 / 25.0
    for k in range(23, 0, -2):  # p z + 1/23, …, p z + 1/3, p z + 1
        p = p * z + 1.0 / k
    return float(e) * 0.6931471805599453 + (2.0 * s) * p


def _lrint(v):
    f = -v if v < 0 else v
    i = int(f)
    frac = f - float(i)
    if frac > 0.5 or (frac == 0.5 and (i & 1)):
        i += 1
    return -i if v < 0 else i


def update_num_iters(p, ep, model_points, max_iters):
    p = min(max(p, 0.0), 1.0)
    ep = min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, DBL_MIN)
    pw = 1.0
    for _ in range(model_points):
        pw = pw * (1.0 - ep)
    den = 1.0 - pw
    if den < DBL_MIN:
        return 0
    num, den = det_log(num), det_log(den)
    if den >= 0 or -num >= max_iters * (-den):
        return max_iters
    return _lrint(num / den)


# ---------------------------------------------------------------------------------------------------------------- sampling
def draw(h, n):
    """The five distinct indices of hypothesis h and the number of duplicate draws it threw away."""
    s = (SEED + h * STRIDE) & M64
    idx, dups = [], 0
    while len(idx) < MODEL:
        s = (s + 0x9E3779B97F4A7C15) & M64
        z = s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        c = (z ^ (z >> 31)) % n
        if c in idx:
            dups += 1
        else:
            idx.append(c)
    return idx, dups


# ------------------------------------------------------------------------------------------------------ the camera and its sums
def _rot(q):
    w, x, y, z = q
    return (1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
            2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
            2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y))


class _Camera:
    def __init__(self, xyz, xy, f, cx, cy):
        self.X, self.Y, self.Z = (np.ascontiguousarray(xyz[:, k], np.float64) for k in range(3))
        self.u, self.v = (np.ascontiguousarray(xy[:, k], np.float64) for k in range(2))
        self.f, self.cx, self.cy = f, cx, cy

    def terms(self, pose, idx, jac):
        """Per point of `idx` one row: the 36 products of H (row-major, upper half meaningful), the 6 of g, e².  Without `jac`
        the e² column alone."""
        q, t = pose
        R = _rot(q)
        X, Y, Z = self.X[idx], self.Y[idx], self.Z[idx]
        rx = R[0] * X + R[1] * Y + R[2] * Z
        ry = R[3] * X + R[4] * Y + R[5] * Z
        rz = R[6] * X + R[7] * Y + R[8] * Z
        px, py, pz = rx + t[0], ry + t[1], rz + t[2]
        iz = 1.0 / pz
        ex = self.f * px * iz + self.cx - self.u[idx]
        ey = self.f * py * iz + self.cy - self.v[idx]
        e2 = ex * ex + ey * ey
        if not jac:
            return e2[:, None]
        a = self.f * iz
        bx = -self.f * px * iz * iz
        by = -self.f * py * iz * iz
        zero = np.zeros_like(a)
        J0 = np.stack([bx * ry, a * rz - bx * rx, -a * ry, a, zero, bx], 1)
        J1 = np.stack([-a * rz + by * ry, -by * rx, a * rx, zero, a, by], 1)
        H = J0[:, :, None] * J0[:, None, :] + J1[:, :, None] * J1[:, None, :]
        g = J0 * ex[:, None] + J1 * ey[:, None]
        return np.concatenate([H.reshape(-1, 36), g, e2[:, None]], 1)

    def test(self, pose, thr2, strict, z_test):
        q, t = pose
        R = _rot(q)
        px = R[0] * self.X + R[1] * self.Y + R[2] * self.Z + t[0]
        py = R[3] * self.X + R[4] * self.Y + R[5] * self.Z + t[1]
        pz = R[6] * self.X + R[7] * self.Y + R[8] * self.Z + t[2]
        front = pz > 0
        iz = 1.0 / pz
        ex = self.f * px * iz + self.cx - self.u
        ey = self.f * py * iz + self.cy - self.v
        e2 = ex * ex + ey * ey
        ok = (e2 < thr2) if strict else (e2 <= thr2)
        return (ok & front if z_test else ok), int((~front).sum())


def _sum_sequential(T):
    s = np.zeros(T.shape[1])
    for row in T:
        s = s + row
    return s


def _sum_tree(T):
    """256 strided partials (each sequential over k = t, t + 256, …), then partial[t] += partial[t + s], s = 128 … 1."""
    m, w = T.shape
    rows = -(-m // 256)
    P = np.zeros((rows * 256, w))
    P[:m] = T
    P = P.reshape(rows, 256, w)
    part = np.zeros((256, w))
    for r in range(rows):
        part = part + P[r]
    s = 128
    while s:
        part = part[:s] + part[s:2 * s]
        s >>= 1
    return part[0]


# ------------------------------------------------------------------------------------------------------------ one LM step
def solve6(H, g, lam, jitter=1e-12):
    """d with (H + λ diag H + jitter I) d = −g by the declared Cholesky, or None.  H: 36 floats, the upper half is read.

    Declared left-looking: element (i, j) is a_ij minus the products l_ik·l_jk one at a time in ascending k, then one division.
    Written here right-looking (once column k is known, its outer product leaves the whole trailing block), which performs the
    same subtractions on each element in the same ascending k, so the bits are those declared; likewise the forward
    substitution by columns.  The backward substitution is declared in ascending k while d is known in descending k, so it
    stays by rows."""
    U = np.array(H, np.float64).reshape(6, 6)
    A = np.triu(U) + np.triu(U, 1).T  # symmetric from the upper half
    A[np.diag_indices(6)] += lam * np.diag(U) + jitter
    L = np.zeros((6, 6))
    for k in range(6):
        if not A[k, k] > 0:
            return None
        L[k, k] = math.sqrt(A[k, k])
        L[k + 1:, k] = A[k + 1:, k] / L[k, k]
        A[k + 1:, k + 1:] -= np.outer(L[k + 1:, k], L[k + 1:, k])
    y = -np.array(g, np.float64)
    for k in range(6):
        y[k] = y[k] / L[k, k]
        y[k + 1:] -= L[k + 1:, k] * y[k]
    d = [0.0] * 6
    for i in range(5, -1, -1):
        v = float(y[i])
        for k in range(i + 1, 6):
            v -= float(L[k, i]) * d[k]
        d[i] = v / float(L[i, i])
    return d


def _qmul(a, q):
    return [a[0] * q[0] - a[1] * q[1] - a[2] * q[2] - a[3] * q[3],
            a[0] * q[1] + a[1] * q[0] + a[2] * q[3] - a[3] * q[2],
            a[0] * q[2] - a[1] * q[3] + a[2] * q[0] + a[3] * q[1],
            a[0] * q[3] + a[1] * q[2] - a[2] * q[1] + a[3] * q[0]]


def _norm4(v):
    return math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3])


def retract(pose, d):
    q, t = pose
    dq = [1.0, 0.5 * d[0], 0.5 * d[1], 0.5 * d[2]]
    nn = _norm4(dq)
    dq = [_div(v, nn) for v in dq]
    nq = _qmul(dq, q)
    n2 = _norm4(nq)
    return [_div(v, n2) for v in nq], [t[0] + d[3], t[1] + d[4], t[2] + d[5]]


def lm_solve(cam, pose, idx, max_it, tree, c, variant=None):
    """The LM driver over the points `idx` from `pose`; `c` is the counter dict of this stage."""
    total = _sum_tree if tree else _sum_sequential
    jitter = 0.0 if variant == "no_jitter" else 1e-12
    idx = np.asarray(idx, np.int64)

    def normal(p):
        s = total(cam.terms(p, idx, True))
        return float(s[42]), s[:36].tolist(), s[36:42].tolist()

    lam = 1e-3
    cost, H, g = normal(pose)
    if cost != cost:
        c["nan_cost"] += 1
    for _ in range(max_it):
        d = solve6(H, g, lam, jitter)
        if d is None:
            c["chol_fail"] += 1
            lam *= 10
            continue
        cand = retract(pose, d)
        c2 = float(total(cam.terms(cand, idx, False))[0])
        if c2 != c2:
            c["nan_cost"] += 1
        if c2 < cost:
            c["accept"] += 1
            q, t = pose
            x2 = ((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]) + 4.0 * ((q[1] * q[1] + q[2] * q[2]) + q[3] * q[3])
            pose = cand
            lam *= 0.1
            if lam < 1e-9 and variant != "no_lam_floor":
                lam = 1e-9
                c["lam_floor"] += 1
            step2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3] + d[4] * d[4] + d[5] * d[5]
            cost, H, g = normal(pose)
            small, rel = step2 < 1e-20, step2 <= REL_STEP2 * x2
            if small and not rel:
                c["exit_abs_alone"] += 1
            if small and variant != "no_abs_stop":
                c["exit_abs"] += 1
                return pose
            if rel:
                c["exit_rel"] += 1
                return pose
        else:
            c["reject"] += 1
            lam *= 10
            if lam > 1e6:
                c["exit_lambda"] += 1
                return pose
    c["exit_cap"] += 1
    return pose


# ---------------------------------------------------------------------------------------------------------------- the call
def pnp_ransac(xyz, xy, focal, cx, cy, rvec, tvec, iterations=100, reproj_err=8.0, confidence=0.99, variant=None):
    """(rvec, tvec, inliers, record).  record: best, niters, counts (of the hypotheses consumed, in order), min / ref (LM counters
    of the minimal solves and of the refinement), and the call's own counters (CALL_COUNTERS)."""
    assert variant is None or variant in VARIANTS, variant
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    n = xyz.shape[0]
    rv = [float(v) for v in np.asarray(rvec, np.float64)]
    tv = [float(v) for v in np.asarray(tvec, np.float64)]
    rec = {"best": -1, "niters": iterations, "counts": [], "min": dict.fromkeys(LM_COUNTERS, 0), "ref": dict.fromkeys(LM_COUNTERS, 0)}
    rec.update(dict.fromkeys(CALL_COUNTERS, 0))
    none = np.zeros(0, np.int32)
    if n < MODEL:
        return np.array(rv), np.array(tv), none, rec
    cam = _Camera(xyz, xy, float(np.float32(focal)), float(np.float32(cx)), float(np.float32(cy)))
    err = np.float32(reproj_err)
    thr2 = float(err * err) if variant == "thr_f32sq" else float(err) * float(err)
    strict, z_test = variant == "thr_strict", variant != "no_z_test"
    guess = (quat_from_rvec(rv), tv)
    best, best_cnt, best_pose, best_mask, niters = -1, 0, None, None, iterations
    h = 0
    with np.errstate(all="ignore"):
        while h < niters:
            idx, dups = draw(h, n)
            rec["dup_draw"] += dups
            pose = lm_solve(cam, guess, idx, 12, variant == "min_tree", rec["min"], variant)
            mask, behind = cam.test(pose, thr2, strict, z_test)
            rec["z_le_0"] += behind
            cnt = int(mask.sum())
            rec["counts"].append(cnt)
            if cnt >= MODEL and cnt == best_cnt:
                rec["tie"] += 1
            if cnt > max(best_cnt, MODEL - 1) or (variant == "tie_replaces" and cnt >= max(best_cnt, MODEL)):
                best, best_cnt, best_pose, best_mask = h, cnt, pose, mask
                if variant != "no_cap":
                    niters = update_num_iters(confidence, (n - best_cnt) / n, MODEL, niters)
            h += 1
        rec["best"], rec["niters"] = best, niters
        if best < 0:
            return np.array(rv), np.array(tv), none, rec
        inl = np.flatnonzero(best_mask)
        q, t = lm_solve(cam, best_pose, inl, 20, variant != "seq_sum", rec["ref"], variant)
    return np.array(rvec_from_quat(q, rec)), np.array(t), inl.astype(np.int32), rec
