"""Independent float64 reference for the window solve (a12: BundleAdjuster::bundle_adjust -> ceres::Solve), numpy only.

Written from SURVEY.md Appendix B (the Ceres trust-region Levenberg-Marquardt loop with its defaults) and the residual of
ReprojectionFactor: gamma = R(q) p / |q|^2 + t, r = f gamma_xy / gamma_z + c - obs.  It shares nothing
with the oracle, the host step control or the kernels: no chunks, no wire format, no declared summation order, geometric
Jacobians (d gamma / d delta = -2 [R p]x for the quaternion Plus of Appendix B, d gamma / d t = I, d gamma / d p = R),
checked against central differences of the residual in tests/test_ba_ref.py.  Non-unit quaternions are accepted and Plus
does not renormalise.

The loop, per iteration, as Ceres' TrustRegionMinimizer runs it with a LevenbergMarquardtStrategy:
  * Jacobi scaling 1 / (1 + |column|) from the FIRST Jacobian, kept for the whole solve;
  * LM diagonal D = sqrt(clamp(diag(Js' Js), 1e-6, 1e32) / radius) of the scaled Jacobian Js, reused after a rejection;
  * y = argmin |Js y - r|^2 + |D y|^2, step = -y, model change = -(Js step) . (r + Js step / 2), delta = step * scale;
  * candidate = Plus(x, delta); parameter tolerance on |x - candidate| (ambient, 7 per pose) <= 1e-8 (|x| + 1e-8), then
    function tolerance |cost - candidate cost| <= 1e-6 cost: both return BEFORE the step is taken;
  * rho = (cost - candidate cost) / model change; rho > 1e-3: accept, radius /= max(1/3, 1 - (2 rho - 1)^3), decrease
    factor = 2; else radius /= decrease factor, decrease factor *= 2;
  * before every iteration: iteration cap (termination 1), gradient tolerance max|J' r| <= 1e-10 (after the start and after
    accepted steps), minimum radius 1e-32.

Three routes for the linear step: "a" dense normal equations, "b" landmark-block Schur complement vectorised in numpy
(with a switch that reverses every summation over observations and landmarks), "c" least squares of the stacked [Js; D].
Only "b" never forms the dense Jacobian; forward, it also evaluates its Jacobian blocks in another, equal form
(jacobian_blocks), because the rounding of the linearisation moves a step by as much as the rounding of the solve does
(measured on the scaled-quaternion scene: candidate cost 1.4e-12 relative between the two evaluations, 1.2e-13 between the
solves of one evaluation).  spread() is the largest difference among the routes for the same quantity: the reference's own
error, from which the tests derive their tolerances (16 x spread, floors COST_FLOOR / POSE_FLOOR / POINT_FLOOR /
RESIDUAL_FLOOR).

Measured spreads of the committed scenes (tests/test_ba_ref.py SCENES; one LM iteration: candidate cost relative, pose
parameters, landmarks in m; whole solve: final cost relative, residuals in px), from the run that produced the table:

k2_one_chunk            2 poses    56 obs  one iteration: cost 1.8e-12  poses 1.1e-13  landmarks 4.2e-11 | 15 iterations: cost 1.4e-14  residuals 1.5e-12
k2_chunk_closes_at_64   2 poses    88 obs  one iteration: cost 1.9e-11  poses 9.7e-14  landmarks 4.1e-11 | 35 iterations: cost 5.2e-14  residuals 1.1e-11
k2_cap_30               2 poses    88 obs  one iteration: cost 1.9e-11  poses 9.7e-14  landmarks 4.1e-11 | 30 iterations: cost 2.3e-13  residuals 2.7e-12
k5_sparse               5 poses   190 obs  one iteration: cost 1.2e-12  poses 1.3e-12  landmarks 3.6e-11 |  8 iterations: cost 1.4e-14  residuals 6.8e-13
k8_sparse               8 poses   346 obs  one iteration: cost 1.9e-13  poses 7.1e-13  landmarks 1.8e-11 | 19 iterations: cost 3.7e-14  residuals 2.6e-11
k6_dense                6 poses   160 obs  one iteration: cost 5.4e-14  poses 1.7e-13  landmarks 3.3e-12 |  7 iterations: cost 7.7e-15  residuals 2.3e-13
k14_sparse             14 poses   255 obs  one iteration: cost 1.4e-12  poses 3.1e-12  landmarks 2.2e-11 | 21 iterations: cost 9.7e-15  residuals 3.3e-12
k14_dense              14 poses   223 obs  one iteration: cost 9.5e-15  poses 4.7e-13  landmarks 2.8e-12 |  4 iterations: cost 1.0e-14  residuals 4.5e-13
many_chunks             3 poses  8177 obs  one iteration: cost 2.3e-11  poses 1.3e-14  landmarks 1.0e-10 |  3 iterations: cost 1.1e-11  residuals 1.1e-09
bad_k3                  3 poses   132 obs  one iteration: cost 9.9e-13  poses 3.8e-12  landmarks 3.2e-11 | 44 iterations: cost 4.3e-13  residuals 3.3e-11
bad_k6                  6 poses   193 obs  one iteration: cost 9.1e-12  poses 2.7e-11  landmarks 9.3e-10 | 34 iterations: cost 1.3e-09  residuals 3.5e-08
bad_k4                  4 poses   128 obs  one iteration: cost 2.8e-12  poses 1.0e-12  landmarks 9.5e-12 |  8 iterations: cost 1.3e-14  residuals 9.1e-13
parameter_tolerance     5 poses   171 obs  one iteration: cost 1.7e-13  poses 2.8e-14  landmarks 1.3e-11 |  8 iterations: cost 8.7e-06  residuals 4.5e-13
optimum                 4 poses    93 obs  one iteration: cost 0.0e+00  poses 0.0e+00  landmarks 0.0e+00 |  1 iterations: cost 0.0e+00  residuals 0.0e+00
clamp                   5 poses   195 obs  one iteration: cost 1.3e-12  poses 9.1e-13  landmarks 6.7e-09 | 11 iterations: cost 1.3e-14  residuals 4.5e-13
structure               5 poses   121 obs  one iteration: cost 4.0e-13  poses 1.3e-12  landmarks 2.7e-11 | 12 iterations: cost 1.8e-14  residuals 3.4e-13
scaled_quaternions      5 poses   111 obs  one iteration: cost 1.7e-12  poses 5.7e-13  landmarks 1.1e-10 | 25 iterations: cost 1.2e-13  residuals 3.1e-12
twice                   4 poses   120 obs  one iteration: cost 1.2e-12  poses 4.8e-13  landmarks 9.9e-11 | 10 iterations: cost 1.9e-14  residuals 3.4e-13
pose_order_reversed     4 poses   118 obs  one iteration: cost 1.1e-12  poses 6.2e-13  landmarks 1.0e-10 | 10 iterations: cost 1.7e-14  residuals 4.5e-13
"""
import numpy as np

F, CX, CY = 718.856, 607.1928, 185.2157

FUNCTION_TOL, GRADIENT_TOL, PARAMETER_TOL = 1e-6, 1e-10, 1e-8
INITIAL_RADIUS, MAX_RADIUS, MIN_RADIUS = 1e4, 1e16, 1e-32
MIN_RELATIVE_DECREASE = 1e-3
MIN_LM_DIAGONAL, MAX_LM_DIAGONAL = 1e-6, 1e32
MAX_INVALID_STEPS = 5

# floors of the tolerances: relative for costs, absolute for pose parameters (quaternion components, metres) and landmarks
# (metres).  A residual is f x / z of such parameters: its floor is the pose floor times the focal length (pixels).
COST_FLOOR, POSE_FLOOR, POINT_FLOOR = 1e-14, 1e-13, 1e-12
RESIDUAL_FLOOR = F * POSE_FLOOR
MARGIN = 16.0
DENSE_LIMIT = 3000  # parameters beyond which only route "b" is run


# ----------------------------------------------------------------------------------------------------------- geometry
def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def rotate(q, p):
    """R(q) p / |q|^2 with R |q|^2 = v v' + (w I + [v]x)^2 (a11), rows of q (.., 4) w-first on rows of p (.., 3)."""
    w, v = q[..., :1], q[..., 1:]
    a = w * p + _cross(v, p)
    b = w * a + _cross(v, a)
    return (v * (v * p).sum(-1, keepdims=True) + b) / (q * q).sum(-1, keepdims=True)


def residuals(poses, points, op, oj, uv, f=F, cx=CX, cy=CY):
    """(M, 2) reprojection residuals; poses (K, 7) world-wrt-camera [qw qx qy qz tx ty tz]."""
    g = rotate(poses[op, :4], points[oj]) + poses[op, 4:]
    return np.stack([f * g[:, 0] / g[:, 2] + cx, f * g[:, 1] / g[:, 2] + cy], 1) - uv


def cost_of(r):
    return 0.5 * float((r * r).sum())


def quat_mul(a, b):
    w1, x1, y1, z1 = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    w2, x2, y2, z2 = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], -1)


def plus_pose(pose, d):
    """Appendix B: q+ = [cos|d|, sin|d| / |d| d] (x) q, no renormalisation; t+ = t + d[3:]."""
    out = pose.copy()
    th = np.linalg.norm(d[:3])
    if th > 0.0:
        qd = np.concatenate([[np.cos(th)], np.sin(th) / th * d[:3]])
        out[:4] = quat_mul(qd, pose[:4])
    out[4:] = pose[4:] + d[3:]
    return out


def rotation_angle(qa, qb):
    """Angle between the rotations of two quaternions (any norms), from the VECTOR part of the relative quaternion: resolves
    angles far below the 1.5e-8 at which an arccos of the trace returns 0."""
    qa, qb = np.asarray(qa, float), np.asarray(qb, float)
    qa, qb = qa / np.linalg.norm(qa), qb / np.linalg.norm(qb)
    rel = quat_mul(qa, qb * np.array([1.0, -1.0, -1.0, -1.0]))
    return 2.0 * float(np.arctan2(np.linalg.norm(rel[1:]), abs(rel[0])))


def jacobian_blocks(poses, points, op, oj, f=F, form="quaternion"):
    """Per observation the 2x6 block of its pose's tangent [delta (3) | t (3)] and the 2x3 block of its landmark.  Two evaluations
    of the same derivative: "quaternion" rotates with the residual's own formula, "matrix" with the explicit rotation matrix of the
    normalised quaternion and the reciprocal depth — the dense routes and the reversed Schur route take the first, the forward Schur
    route the second, so that the routes (on large scenes: the two Schur routes) differ in the rounding of the linearisation as well
    as in that of the solve."""
    q = poses[op, :4]
    m = len(op)
    if form == "matrix":
        w, x, y, z = (q / np.sqrt((q * q).sum(1))[:, None]).T
        rot = np.empty((m, 3, 3))
        rot[:, 0, 0], rot[:, 0, 1], rot[:, 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)
        rot[:, 1, 0], rot[:, 1, 1], rot[:, 1, 2] = 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)
        rot[:, 2, 0], rot[:, 2, 1], rot[:, 2, 2] = 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)
        rx = np.einsum("mab,mb->ma", rot, points[oj])
    else:
        rx = rotate(q, points[oj])
        rot = np.stack([rotate(q, np.broadcast_to(e, (m, 3))) for e in np.eye(3)], 2)  # columns R e_i
    g = rx + poses[op, 4:]
    proj = np.zeros((m, 2, 3))
    if form == "matrix":
        iz = 1.0 / g[:, 2]
        proj[:, 0, 0] = proj[:, 1, 1] = f * iz
        proj[:, 0, 2], proj[:, 1, 2] = -(f * iz) * (g[:, 0] * iz), -(f * iz) * (g[:, 1] * iz)
    else:
        proj[:, 0, 0] = proj[:, 1, 1] = f / g[:, 2]
        proj[:, 0, 2], proj[:, 1, 2] = -f * g[:, 0] / g[:, 2] ** 2, -f * g[:, 1] / g[:, 2] ** 2
    skew = np.zeros((m, 3, 3))  # -2 [R p]x
    skew[:, 0, 1], skew[:, 0, 2] = 2 * rx[:, 2], -2 * rx[:, 1]
    skew[:, 1, 0], skew[:, 1, 2] = -2 * rx[:, 2], 2 * rx[:, 0]
    skew[:, 2, 0], skew[:, 2, 1] = 2 * rx[:, 1], -2 * rx[:, 0]
    return np.concatenate([proj @ skew, proj], 2), proj @ rot


# ----------------------------------------------------------------------------------------------------- linearisations
class _Index:
    """Tangent layout [6 per free pose (1 .. K-1) | 3 per observed landmark]; the oldest pose is constant."""

    def __init__(self, K, op, oj):
        self.K, self.op, self.oj = K, np.asarray(op, np.int64), np.asarray(oj, np.int64)
        self.lms = np.unique(self.oj)
        self.n = 6 * (K - 1)
        self.size = self.n + 3 * len(self.lms)
        self.li = np.searchsorted(self.lms, self.oj)
        self.free = self.op > 0
        self.pi = self.op - 1


class _Dense:
    def __init__(self, ix, a, b, route):
        m = len(ix.op)
        J = np.zeros((2 * m, ix.size))
        rows = np.arange(m)
        for row in range(2):
            for c in range(6):
                J[2 * rows[ix.free] + row, 6 * ix.pi[ix.free] + c] = a[ix.free, row, c]
            for c in range(3):
                J[2 * rows + row, ix.n + 3 * ix.li + c] = b[:, row, c]
        self.J, self.route = J, route

    def scaled(self, s):
        out = object.__new__(_Dense)
        out.J, out.route = self.J * s, self.route
        return out

    def colnorm2(self):
        return (self.J * self.J).sum(0)

    def jt(self, r):
        return self.J.T @ r.ravel()

    def apply(self, s):
        return (self.J @ s).reshape(-1, 2)

    def solve(self, d, r):
        if self.route == "a":
            return np.linalg.solve(self.J.T @ self.J + np.diag(d * d), self.J.T @ r.ravel())
        stacked = np.concatenate([self.J, np.diag(d)], 0)
        return np.linalg.lstsq(stacked, np.concatenate([r.ravel(), np.zeros(len(d))]), rcond=None)[0]


class _Schur:
    def __init__(self, ix, a, b, reverse):
        self.ix, self.a, self.b, self.reverse = ix, a, b, reverse
        self.o = np.arange(len(ix.op))[::-1] if reverse else np.arange(len(ix.op))  # order of every sum over observations
        self.of = self.o[ix.free[self.o]]

    def scaled(self, s):
        ix = self.ix
        sp, sl = s[:ix.n].reshape(-1, 6), s[ix.n:].reshape(-1, 3)
        a = self.a.copy()
        a[ix.free] *= sp[ix.pi[ix.free]][:, None, :]
        return _Schur(ix, a, self.b * sl[ix.li][:, None, :], self.reverse)

    def _gather(self, vp, vl):
        ix = self.ix
        p, l = np.zeros((ix.K - 1,) + vp.shape[1:]), np.zeros((len(ix.lms),) + vl.shape[1:])
        np.add.at(p, ix.pi[self.of], vp[self.of])
        np.add.at(l, ix.li[self.o], vl[self.o])
        return p, l

    def colnorm2(self):
        p, l = self._gather((self.a ** 2).sum(1), (self.b ** 2).sum(1))
        return np.concatenate([p.ravel(), l.ravel()])

    def jt(self, r):
        p, l = self._gather(np.einsum("mab,ma->mb", self.a, r), np.einsum("mab,ma->mb", self.b, r))
        return np.concatenate([p.ravel(), l.ravel()])

    def apply(self, s):
        ix = self.ix
        sp, sl = s[:ix.n].reshape(-1, 6), s[ix.n:].reshape(-1, 3)
        out = np.einsum("mab,mb->ma", self.b, sl[ix.li])
        out[ix.free] += np.einsum("mab,mb->ma", self.a[ix.free], sp[ix.pi[ix.free]])
        return out

    def solve(self, d, r):
        ix, a, b = self.ix, self.a, self.b
        nf, nl = ix.K - 1, len(ix.lms)
        dp, dl = d[:ix.n], d[ix.n:].reshape(-1, 3)
        u, v = self._gather(np.einsum("mab,mac->mbc", a, a), np.einsum("mab,mac->mbc", b, b))
        bp, bl = self._gather(np.einsum("mab,ma->mb", a, r), np.einsum("mab,ma->mb", b, r))
        w = np.zeros((nl, nf, 6, 3))
        np.add.at(w, (ix.li[self.of], ix.pi[self.of]), np.einsum("mab,mac->mbc", a, b)[self.of])
        v = v + np.einsum("lb,bc->lbc", dl * dl, np.eye(3))
        vinv = np.linalg.inv(v)
        w = w.reshape(nl, ix.n, 3)
        y = w @ vinv
        lo = slice(None, None, -1) if self.reverse else slice(None)
        S = np.zeros((ix.n, ix.n))
        for k in range(nf):
            S[6 * k:6 * k + 6, 6 * k:6 * k + 6] = u[k]
        S = S + np.diag(dp * dp) - np.einsum("lia,lja->ij", y[lo], w[lo])
        rhs = bp.ravel() - np.einsum("lia,la->i", y[lo], bl[lo])
        yp = np.linalg.solve(S, rhs)
        yl = np.einsum("lab,lb->la", vinv, bl - np.einsum("lia,i->la", w, yp))
        return np.concatenate([yp, yl.ravel()])


def linearize(poses, points, op, oj, route="a", reverse=False, f=F):
    ix = _Index(len(poses), op, oj)
    a, b = jacobian_blocks(poses, points, ix.op, ix.oj, f, "matrix" if route == "b" and not reverse else "quaternion")
    a[~ix.free] = 0.0
    return ix, (_Schur(ix, a, b, reverse) if route == "b" else _Dense(ix, a, b, route))


# -------------------------------------------------------------------------------------------------------------- solve
class Trace(list):
    """One dict per LM iteration (cost, candidate_cost, model_change, rho, radius, decrease_factor, accepted, clamped,
    terminated, gradient_max, step_norm, x_norm) plus the summary of the solve; gradient_start is max|J' r| at the initial state."""
    iterations = successful_steps = termination = 0
    why = None
    initial_cost = final_cost = 0.0


def _ambient(poses, points, ix):
    return np.concatenate([poses[1:].ravel(), points[ix.lms].ravel()])


def solve(problem, max_iterations=50, route="a", reverse=False, f=F, cx=CX, cy=CY):
    """LM solve of problem (dict: poses0, points0, op, oj, uv).  Returns (poses, points, Trace).  Trace.iterations counts the passes
    of the loop entered (the one on which a tolerance fired included; len(trace) are those that computed a step),
    Trace.successful_steps the accepted ones;
    Trace.termination 0 convergence, 1 iteration cap, 2 failure; Trace.why gradient / function / parameter / iterations / radius /
    failure."""
    poses, points = np.array(problem["poses0"], float), np.array(problem["points0"], float)
    op, oj, uv = np.asarray(problem["op"], np.int64), np.asarray(problem["oj"], np.int64), np.asarray(problem["uv"], float)
    tr = Trace()
    r = residuals(poses, points, op, oj, uv, f, cx, cy)
    cost = cost_of(r)
    tr.initial_cost = cost
    ix, lin = linearize(poses, points, op, oj, route, reverse, f)
    scale = 1.0 / (1.0 + np.sqrt(lin.colnorm2()))
    gmax = float(np.abs(lin.jt(r)).max())
    tr.gradient_start = gmax
    lin = lin.scaled(scale)
    x = _ambient(poses, points, ix)
    radius, decrease, reuse, diag, check_gradient, invalid = INITIAL_RADIUS, 2.0, False, None, True, 0
    while True:
        if len(tr) >= max_iterations:
            tr.termination, tr.why = 1, "iterations"
            break
        if check_gradient and gmax <= GRADIENT_TOL:
            tr.termination, tr.why = 0, "gradient"
            break
        if radius <= MIN_RADIUS:
            tr.termination, tr.why = 0, "radius"
            break
        if not reuse:
            raw = lin.colnorm2()
            clamped = int((raw < MIN_LM_DIAGONAL).sum())
            diag = np.clip(raw, MIN_LM_DIAGONAL, MAX_LM_DIAGONAL)
        d = np.sqrt(diag / radius)
        step = -lin.solve(d, r)
        js = lin.apply(step)
        model = -float((js * (r + js / 2.0)).sum())
        it = dict(cost=cost, candidate_cost=None, model_change=model, rho=None, radius=radius, decrease_factor=decrease,
                  accepted=False, clamped=clamped, terminated=None, gradient_max=gmax)
        tr.append(it)
        check_gradient = False
        if not (model > 0.0) or not np.isfinite(step).all():
            invalid += 1
            if invalid >= MAX_INVALID_STEPS:
                it["terminated"] = tr.why = "failure"
                tr.termination = 2
                break
            radius, decrease, reuse = radius / decrease, decrease * 2.0, True
            continue
        invalid = 0
        delta = step * scale
        cposes, cpoints = poses.copy(), points.copy()
        for k in range(1, len(poses)):
            cposes[k] = plus_pose(poses[k], delta[6 * (k - 1):6 * k])
        cpoints[ix.lms] = points[ix.lms] + delta[ix.n:].reshape(-1, 3)
        rc = residuals(cposes, cpoints, op, oj, uv, f, cx, cy)
        ccost = cost_of(rc)
        if not np.isfinite(ccost):
            ccost = np.finfo(float).max
        it["candidate_cost"] = ccost
        xc = _ambient(cposes, cpoints, ix)
        it["step_norm"], it["x_norm"] = float(np.linalg.norm(x - xc)), float(np.linalg.norm(x))
        it["rho"] = rho = (cost - ccost) / model
        if it["step_norm"] <= PARAMETER_TOL * (it["x_norm"] + PARAMETER_TOL):
            it["terminated"] = tr.why = "parameter"
            break
        if abs(cost - ccost) <= FUNCTION_TOL * cost:
            it["terminated"] = tr.why = "function"
            break
        if rho > MIN_RELATIVE_DECREASE:
            it["accepted"] = True
            tr.successful_steps += 1
            poses, points, r, cost, x = cposes, cpoints, rc, ccost, xc
            ix, lin = linearize(poses, points, op, oj, route, reverse, f)
            gmax = float(np.abs(lin.jt(r)).max())
            lin = lin.scaled(scale)
            radius = min(MAX_RADIUS, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
            decrease, reuse, check_gradient = 2.0, False, True
        else:
            radius, decrease, reuse = radius / decrease, decrease * 2.0, True
    # the summary's convention (svo_ba_summary): passes of the loop ENTERED — the gradient and radius tests are made on entering a
    # pass, so a solve that ends on the gradient test at the start reports one iteration and no step; the cap ends the loop itself
    tr.iterations, tr.final_cost = len(tr) + (1 if tr.why in ("gradient", "radius") else 0), cost
    return poses, points, tr


# ------------------------------------------------------------------------------------------------------------- spread
def routes_for(problem):
    size = 6 * (len(problem["poses0"]) - 1) + 3 * len(np.unique(problem["oj"]))
    if size <= DENSE_LIMIT:
        return (("a", False), ("b", False), ("b", True), ("c", False))
    return (("b", False), ("b", True))


_CACHE = {}


def route_solves(problem, max_iterations):
    """[(poses, points, Trace)] of every available route; cached on the problem dict itself."""
    key = (id(problem), max_iterations)
    if key not in _CACHE:
        _CACHE[key] = (problem, [solve(problem, max_iterations, route, rev) for route, rev in routes_for(problem)])
    return _CACHE[key][1]


def reference(problem, max_iterations):
    """The main route's solve (dense normal equations where they fit, else the Schur route)."""
    return route_solves(problem, max_iterations)[0]


def _pairs(vals):
    return max((float(np.max(np.abs(np.asarray(a) - np.asarray(b)))) for i, a in enumerate(vals) for b in vals[i + 1:]), default=0.0)


def spread(problem, quantity, max_iterations=1):
    """Largest difference among the routes after max_iterations: "cost" (final cost, relative), "initial_cost" (relative), "poses"
    (free pose parameters), "points" (observed landmarks, m), "residuals" (px, recomputed at each route's returned state)."""
    sols = route_solves(problem, max_iterations)
    if quantity == "cost":
        c = [s[2].final_cost for s in sols]
        return _pairs(c) / max(abs(c[0]), np.finfo(float).tiny)
    if quantity == "initial_cost":
        c = [s[2].initial_cost for s in sols]
        return _pairs(c) / max(abs(c[0]), np.finfo(float).tiny)
    if quantity == "poses":
        return _pairs([s[0][1:] for s in sols])
    if quantity == "points":
        seen = np.unique(problem["oj"])
        return _pairs([s[1][seen] for s in sols])
    if quantity == "residuals":
        return _pairs([residuals(s[0], s[1], problem["op"], problem["oj"], problem["uv"]) for s in sols])
    raise KeyError(quantity)


def tolerance(problem, quantity, max_iterations=1):
    """16 x spread, not below the floor of the quantity (costs: relative)."""
    floor = {"cost": COST_FLOOR, "initial_cost": COST_FLOOR, "poses": POSE_FLOOR, "points": POINT_FLOOR, "residuals": RESIDUAL_FLOOR}[quantity]
    return max(MARGIN * spread(problem, quantity, max_iterations), floor)
