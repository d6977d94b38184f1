"""a12 window solve against an INDEPENDENT reference (tests/ba_ref.py: dense float64 numpy LM written from SURVEY Appendix B,
no Schur, no chunks, no wire format) on scenes that reach every decision of the loop.  The oracle (oracle/ora_ba.cpp), the
host step control (host/lm.cpp) and the kernels were written from one reading of Ceres and are changed together; an error in
that reading passes every bit-for-bit test.  Compared here: after ONE LM iteration the costs, every free pose parameter and
every observed landmark; after whole solves only gauge-free quantities (the counts, the final cost, the residual vector at
the returned state) — the free scale of the problem moves low-parallax landmarks by millimetres between correct solvers.
Every tolerance is 16 x the spread of the reference's own solve routes for that quantity on that scene, computed at test time
(floors: ba_ref.COST_FLOOR, POSE_FLOOR, POINT_FLOOR, RESIDUAL_FLOOR).

What these tests found in the bulk accumulation paths when they were written (fixed in csrc/ba.hip with them):
  * atomics, scene "twice": two observations of one landmark by one pose entered the pose's diagonal block of S once, not both ways,
    and a landmark whose observations were not in pose order wrote lower blocks the device step control never reads — after one
    iteration the poses were 2.6e-2 and the landmarks 7.5 m from the reference's (tolerances 7.7e-12 and 1.6e-9 m);
  * mfma, scene "bad_k6": Z came from the Cholesky factor of the INVERTED landmark block and g_red from the inverse itself — the cost
    after one iteration missed by 5.6e-4 (tolerance 4.9e-4), poses 3.7e-10 (4.3e-10); the atomics path, on the oracle's cofactor
    inverse, was 2.0e-6 .. 2.95e-6 from the cost after four iterations over five runs (tolerance 2.9e-6).  Both now eliminate through
    the factor of the block itself: 5.3e-6 / 7.3e-12 and 2.4e-8 .. 1.1e-7.
The deterministic forms keep the oracle's declared arithmetic; their worst figure is bad_k6's cost after four iterations, 2.5e-6 of
2.9e-6."""
import os

import numpy as np
import pytest

import ba_problem as BP
import ba_ref as R
import oracle_lib as O

BAD = dict(pose_sigma=(1.5, 0.2), pt_sigma=0.3)


def _sorted(p):
    o = np.argsort(p["oj"], kind="stable")
    p["op"], p["oj"], p["uv"] = np.ascontiguousarray(p["op"][o], np.int32), np.ascontiguousarray(p["oj"][o], np.int32), np.ascontiguousarray(p["uv"][o])
    return p


def _project(p, k, X, f=BP.F, cx=BP.CX, cy=BP.CY):
    return R.residuals(p["poses_gt"], np.asarray(X, float)[None], np.array([k]), np.array([0]), np.zeros((1, 2)), f, cx, cy)[0]


def _add_landmark(p, X, X0, views, rng, noise=0.5):
    """A landmark at X (started at X0) seen by the poses in views (a pose may appear twice); appended, so the order stays landmark-major."""
    j = len(p["points0"])
    p["points_gt"] = np.vstack([p["points_gt"], X]); p["points0"] = np.vstack([p["points0"], X0])
    for k in views:
        p["op"] = np.append(p["op"], np.int32(k)); p["oj"] = np.append(p["oj"], np.int32(j))
        p["uv"] = np.vstack([p["uv"], _project(p, k, X) + rng.normal(0, noise, 2)])
    return j


def _plain(seed, K, N, **kw):
    return lambda: BP.make_problem(seed, K, N, **kw)


def _clamp():
    """A landmark 2,000 km away seen by every pose: its three scaled columns have squared norm below 1e-6 (f / z = 3.6e-4 px/m)."""
    p = BP.make_problem(1, 5, 60)
    rng = np.random.default_rng(101)
    X = np.array([3.0e3, -1.0e3, 2.0e6])
    _add_landmark(p, X, X + rng.normal(0, 0.1, 3), range(5), rng)
    return _sorted(p)


def _structure():
    """A landmark seen only by the fixed pose, one seen by the fixed pose and one free pose, unobserved landmarks in the index space
    (before, between and after the observed ones) and input quaternions scaled by 0.6 .. 1.7."""
    p = BP.make_problem(33, 5, 40)
    rng = np.random.default_rng(102)
    X = np.array([1.5, 0.4, 22.0]); _add_landmark(p, X, X + rng.normal(0, 0.1, 3), [0], rng)
    X = np.array([-2.0, -0.6, 18.0]); _add_landmark(p, X, X + rng.normal(0, 0.1, 3), [0, 3], rng)
    n0 = len(p["points0"])
    new_index, pts, gt = [], [], []
    for j in range(n0):
        if j % 7 == 0:
            for _ in range(1 + j % 3):
                pts.append(rng.normal(size=3) * 50.0); gt.append(pts[-1])
        new_index.append(len(pts)); pts.append(p["points0"][j]); gt.append(p["points_gt"][j])
    for _ in range(5):
        pts.append(rng.normal(size=3) * 50.0); gt.append(pts[-1])
    p["points0"], p["points_gt"] = np.array(pts), np.array(gt)
    p["oj"] = np.array([new_index[j] for j in p["oj"]], np.int32)
    s = np.linspace(0.6, 1.7, 5)
    p["poses0"] = p["poses0"].copy(); p["poses0"][:, :4] *= s[:, None]
    return _sorted(p)


def _scaled_quaternions():
    """Input quaternions of norm 0.6 .. 1.7: the residual divides by |q|^2 and Plus does not renormalise."""
    p = BP.make_problem(32, 5, 40)
    p["poses0"] = p["poses0"].copy(); p["poses0"][:, :4] *= np.linspace(0.6, 1.7, 5)[:, None]
    return p


def _twice():
    """Two landmarks observed twice by one free pose (two detections of one point): both observations count."""
    p = BP.make_problem(8, 4, 40)
    rng = np.random.default_rng(103)
    for j, k in ((3, 2), (17, 1)):
        p["op"] = np.append(p["op"], np.int32(k)); p["oj"] = np.append(p["oj"], np.int32(j))
        p["uv"] = np.vstack([p["uv"], _project(p, k, p["points_gt"][j]) + rng.normal(0, 0.5, 2)])
    return _sorted(p)


def _pose_order_reversed():
    """Every landmark's observations from the newest pose to the oldest (svo_ba_load_problem asks for landmark order only)."""
    p = BP.make_problem(8, 4, 40)
    o = np.lexsort((-p["op"], p["oj"]))
    p["op"], p["oj"], p["uv"] = np.ascontiguousarray(p["op"][o]), np.ascontiguousarray(p["oj"][o]), np.ascontiguousarray(p["uv"][o])
    return p


def _optimum():
    """A noise-free problem started at its optimum: the observations are the reference's own projections of the true state, so the
    gradient is rounding (|J' r| <= 1e-10 with a margin of orders) and the solve ends before its first step."""
    p = BP.make_problem(2, 4, 40, noise=0.0)
    p["poses0"], p["points0"] = p["poses_gt"].copy(), p["points_gt"].copy()
    p["uv"] = R.residuals(p["poses_gt"], p["points_gt"], p["op"], p["oj"], np.zeros_like(p["uv"]))
    return p


# name -> (builder, max_iterations, the decisions its reference trace must reach)
SCENES = {
    "k2_one_chunk": (_plain(7, 2, 30), 50, ("one_chunk",)),
    "k2_chunk_closes_at_64": (_plain(6, 2, 50), 50, ("closes_at_64", "reject_then_accept", "function")),
    "k2_cap_30": (_plain(6, 2, 50), 30, ("iterations",)),
    "k5_sparse": (_plain(1, 5, 60), 50, ("chunks_3_6", "function", "rho_both")),
    "k8_sparse": (_plain(3, 8, 80), 50, ("chunks_3_6", "reject_then_accept")),
    "k6_dense": (_plain(5, 6, 30, dense=True), 50, ("chunks_3_6", "function")),
    "k14_sparse": (_plain(4, 14, 40), 50, ("chunks_3_6",)),
    "k14_dense": (_plain(9, 14, 20, dense=True), 50, ("chunks_3_6",)),
    "many_chunks": (_plain(46, 3, 3600), 3, ("grouped", "rho_both")),
    "bad_k3": (_plain(23, 3, 60, **BAD), 50, ("two_rejections", "rho_both")),
    "bad_k6": (_plain(22, 6, 60, pose_sigma=(2.5, 0.3), pt_sigma=0.5), 50, ("function",)),
    "bad_k4": (_plain(31, 4, 50, pose_sigma=(1.0, 0.1), pt_sigma=0.5), 50, ("function",)),
    "parameter_tolerance": (_plain(12, 5, 60, noise=0.0, pt_sigma=0.05), 50, ("parameter",)),
    "optimum": (_optimum, 50, ("gradient",)),
    "clamp": (_clamp, 50, ("clamped",)),
    "structure": (_structure, 50, ("function",)),
    "scaled_quaternions": (_scaled_quaternions, 50, ("function",)),
    "twice": (_twice, 50, ("function",)),
    "pose_order_reversed": (_pose_order_reversed, 50, ("function",)),
}
BADLY_STARTED = ("bad_k3", "bad_k6", "bad_k4")
_BUILT = {}


def scene(name):
    """The scene's problem, built once and never changed (ba_ref caches its route solves on it)."""
    if name not in _BUILT:
        _BUILT[name] = SCENES[name][0]()
    return _BUILT[name], SCENES[name][1]


def chunk_lengths(oj):
    """Observations per wave chunk: whole landmarks, greedily, at most 64 (host/ba_layout.h)."""
    out, cur = [], 0
    for n in np.bincount(oj)[np.bincount(oj) > 0]:
        if cur + n > 64:
            out.append(cur); cur = 0
        cur += n
    return out + [cur]


# ------------------------------------------------------------------------------------------------------- comparison
class Summary:
    def __init__(self, iterations, successful_steps, termination, initial_cost, final_cost):
        self.iterations, self.successful_steps, self.termination = int(iterations), int(successful_steps), int(termination)
        self.initial_cost, self.final_cost = float(initial_cost), float(final_cost)

    def counts(self):
        return (self.iterations, self.successful_steps, self.termination)


def cost_tolerance(p, quantity, max_iterations, cost):
    """Absolute tolerance of a cost: 16 x spread (floor 1e-14), both relative, and never below the cost of residuals that are all at
    their own floor — what compares costs of about 0 (a noise-free problem at its optimum)."""
    return max(R.tolerance(p, quantity, max_iterations) * abs(cost), len(p["op"]) * R.RESIDUAL_FLOOR ** 2)


def _figure(label, what, got, tol):
    print("%-40s %-28s %.3e (tolerance %.3e)" % (label, what, got, tol))
    return got <= tol


def compare_costs_after(name, run, label, k):
    """The counts and the cost after k iterations against the reference."""
    p, _ = scene(name)
    poses, pts, s = run(p, k)
    _, _, tr = R.reference(p, k)
    assert s.counts() == (tr.iterations, tr.successful_steps, tr.termination), (label, k, s.counts(), tr.why)
    assert _figure(label, "cost after %d iterations" % k, abs(s.final_cost - tr.final_cost), cost_tolerance(p, "cost", k, tr.final_cost))


def compare_with_reference(name, run, label):
    """run(problem, max_iterations) -> (poses, points, Summary) against the reference: section 4 of the issue."""
    p, mi = scene(name)
    seen = np.unique(p["oj"])
    unseen = np.setdiff1d(np.arange(len(p["points0"])), seen)
    ok = []
    # ---- one LM iteration: the free parameters themselves
    poses, pts, s = run(p, 1)
    rp, rx, tr = R.reference(p, 1)
    assert s.counts() == (tr.iterations, tr.successful_steps, tr.termination), (label, "one iteration", s.counts(), tr.why)
    ok.append(_figure(label, "initial cost", abs(s.initial_cost - tr.initial_cost), cost_tolerance(p, "initial_cost", 1, tr.initial_cost)))
    ok.append(_figure(label, "cost after one iteration", abs(s.final_cost - tr.final_cost), cost_tolerance(p, "cost", 1, tr.final_cost)))
    ok.append(_figure(label, "free pose parameters", np.abs(poses[1:] - rp[1:]).max(), R.tolerance(p, "poses", 1)))
    ok.append(_figure(label, "observed landmarks (m)", np.abs(pts[seen] - rx[seen]).max(), R.tolerance(p, "points", 1)))
    ok.append(_figure(label, "largest rotation difference (rad)", max(R.rotation_angle(a, b) for a, b in zip(poses[1:, :4], rp[1:, :4])),
                      4.0 * R.tolerance(p, "poses", 1) / np.linalg.norm(p["poses0"][1:, :4], axis=1).min()))  # |dq| <= 2 tol, angle <= 2 |dq| / |q|
    assert np.array_equal(poses[0], p["poses0"][0]) and np.array_equal(pts[unseen], p["points0"][unseen]), label
    # ---- the whole solve: gauge-free quantities only
    poses, pts, s = run(p, mi)
    rp, rx, tr = R.reference(p, mi)
    assert s.counts() == (tr.iterations, tr.successful_steps, tr.termination), (label, "whole solve", s.counts(), tr.why)
    ok.append(_figure(label, "initial cost", abs(s.initial_cost - tr.initial_cost), cost_tolerance(p, "initial_cost", mi, tr.initial_cost)))
    ok.append(_figure(label, "final cost", abs(s.final_cost - tr.final_cost), cost_tolerance(p, "cost", mi, tr.final_cost)))
    r_got = R.residuals(poses, pts, p["op"], p["oj"], p["uv"])
    ok.append(_figure(label, "residuals at the returned state (px)", np.abs(r_got - R.residuals(rp, rx, p["op"], p["oj"], p["uv"])).max(),
                      R.tolerance(p, "residuals", mi)))
    assert np.array_equal(poses[0], p["poses0"][0]) and np.array_equal(pts[unseen], p["points0"][unseen]), label
    assert all(ok), label


# -------------------------------------------------------------------------------------------------------- CPU tests
def test_reference_jacobians_match_central_differences():
    """Both evaluations of the geometric Jacobian against central differences of the reference's residual through Plus, on non-unit
    quaternions.  h = 1e-6: rounding eps |u| / h = 3e-7 px per unit, truncation h^2 |J'''| / 6 below that — 1e-5 + 1e-7 |J|."""
    rng = np.random.default_rng(7)
    p = BP.make_problem(3, 4, 40)
    poses = p["poses0"].copy(); poses[:, :4] *= rng.uniform(0.6, 1.7, 4)[:, None]
    pts, op, oj, uv = p["points0"], p["op"].astype(np.int64), p["oj"].astype(np.int64), p["uv"]
    h = 1e-6
    for form in ("quaternion", "matrix"):
        a, b = R.jacobian_blocks(poses, pts, op, oj, form=form)
        for c in range(6):
            d = np.zeros(6); d[c] = h
            plus = np.array([R.plus_pose(q, d) for q in poses]); minus = np.array([R.plus_pose(q, -d) for q in poses])
            num = (R.residuals(plus, pts, op, oj, uv) - R.residuals(minus, pts, op, oj, uv)) / (2 * h)
            assert (np.abs(num - a[:, :, c]) <= 1e-5 + 1e-7 * np.abs(a[:, :, c])).all(), (form, c, np.abs(num - a[:, :, c]).max())
        for c in range(3):
            d = np.zeros(3); d[c] = h
            num = (R.residuals(poses, pts + d, op, oj, uv) - R.residuals(poses, pts - d, op, oj, uv)) / (2 * h)
            assert (np.abs(num - b[:, :, c]) <= 1e-5 + 1e-7 * np.abs(b[:, :, c])).all(), (form, c, np.abs(num - b[:, :, c]).max())


def test_rotation_angle_resolves_what_arccos_cannot():
    q = np.array([0.9, 0.1, -0.3, 0.2])
    for angle in (1e-3, 1e-8, 1e-12):
        dq = np.array([np.cos(angle / 2), np.sin(angle / 2), 0.0, 0.0])
        assert abs(R.rotation_angle(R.quat_mul(dq, q), 1.7 * q) - angle) <= 1e-15 + 1e-9 * angle  # 4 ulp of the unit quaternions
        assert abs(R.rotation_angle(-R.quat_mul(dq, q), q) - angle) <= 1e-15 + 1e-9 * angle        # q and -q are one rotation
    assert BP.pose_error(np.r_[R.quat_mul(dq, q), 0, 0, 0][None], np.r_[q, 0, 0, 0][None])[1] == 0.0  # (why the new tests do not use it)


SMALL = [n for n in SCENES if n != "many_chunks"]


@pytest.mark.parametrize("name", list(SCENES))
def test_reference_routes_agree(name):
    """Dense normal equations, the Schur complement (both summation orders) and least squares of the stacked system take the same
    decisions on every scene and the same step to rounding: with unit-norm scaled columns and an LM diagonal of at least 1e-6 / radius
    the condition number of the damped normal equations is below 1e10 per unit of step, so 1e-6 of the parameter's size bounds a
    correct route; a wrong one misses by orders."""
    p, mi = scene(name)
    sols = R.route_solves(p, mi)
    assert len(sols) == (2 if name == "many_chunks" else 4)
    for _, _, tr in sols[1:]:
        assert (tr.iterations, tr.successful_steps, tr.termination, tr.why) == (sols[0][2].iterations, sols[0][2].successful_steps, sols[0][2].termination, sols[0][2].why)
        assert [i["accepted"] for i in tr] == [i["accepted"] for i in sols[0][2]]
    size = max(1.0, float(np.abs(p["points0"][np.unique(p["oj"])]).max()))
    assert R.spread(p, "cost", 1) <= 1e-6 and R.spread(p, "poses", 1) <= 1e-6 and R.spread(p, "points", 1) <= 1e-6 * size
    assert R.spread(p, "cost", mi) <= 1e-6 or sols[0][2].final_cost < 1e-12


def _rejections(tr):
    return "".join("A" if i["accepted"] else "r" for i in tr if i["terminated"] is None)


@pytest.mark.parametrize("name", list(SCENES))
def test_scene_reaches_its_decisions(name):
    """The reference's trace of every scene reaches the decisions the scene is there for, with margins rounding cannot cross:
    |rho - 1e-3| > 1e-6 at every decided step, the relative cost change more than 1e-9 away from the function tolerance, the step
    norm a factor 3 away from the parameter tolerance, the gradient a factor 100 above its tolerance wherever it is tested."""
    p, mi = scene(name)
    _, _, tr = R.reference(p, mi)
    want = SCENES[name][2]
    lens = chunk_lengths(p["oj"])
    assert (np.diff(p["oj"]) >= 0).all() and np.bincount(p["oj"]).max() <= 64  # what svo_ba_load_problem accepts
    for i in tr:
        if i["rho"] is not None:
            assert abs(i["rho"] - R.MIN_RELATIVE_DECREASE) > 1e-6
            assert abs(abs(i["cost"] - i["candidate_cost"]) / i["cost"] - R.FUNCTION_TOL) > 1e-9
            ratio = i["step_norm"] / (R.PARAMETER_TOL * (i["x_norm"] + R.PARAMETER_TOL))
            assert ratio > 3.0 or ratio < 1.0 / 3.0
        assert i["gradient_max"] > 100 * R.GRADIENT_TOL
    decided = {
        "one_chunk": lambda: len(lens) == 1,
        "closes_at_64": lambda: lens[0] == 64 and len(lens) > 1,
        "chunks_3_6": lambda: 3 <= len(lens) <= 6,
        "grouped": lambda: 128 < len(lens) <= 256 and len(p["poses0"]) == 3 and mi <= 3,
        "reject_then_accept": lambda: "ArA" in _rejections(tr),
        "two_rejections": lambda: any(not a["accepted"] and not b["accepted"] and (a["decrease_factor"], b["decrease_factor"]) == (2.0, 4.0)
                                      and b["radius"] == a["radius"] / 2.0 and b["clamped"] == a["clamped"] for a, b in zip(tr, tr[1:])),
        "rho_both": lambda: any(i["accepted"] and i["rho"] >= 0.9368 for i in tr) and any(i["accepted"] and i["rho"] < 0.9368 for i in tr),
        "function": lambda: (tr.why, tr.termination) == ("function", 0) and tr.iterations < mi,
        "parameter": lambda: (tr.why, tr.termination) == ("parameter", 0),
        "gradient": lambda: (tr.why, tr.termination, tr.iterations, tr.successful_steps, len(tr)) == ("gradient", 0, 1, 0, 0) and tr.gradient_start < 1e-3 * R.GRADIENT_TOL,
        "iterations": lambda: (tr.why, tr.termination, tr.iterations) == ("iterations", 1, mi),
        "clamped": lambda: all(i["clamped"] == 3 for i in tr),
    }
    for w in want:
        assert decided[w](), (name, w, _rejections(tr), lens[:4])
    if name == "structure":
        cnt = {j: sorted(p["op"][p["oj"] == j]) for j in np.unique(p["oj"])}
        assert [0] in cnt.values() and [0, 3] in cnt.values() and len(cnt) < len(p["points0"]) and min(cnt) > 0 and max(cnt) < len(p["points0"]) - 1
        assert np.allclose(np.linalg.norm(p["poses0"][:, :4], axis=1), np.linspace(0.6, 1.7, 5), atol=1e-3)
    if name == "twice":
        assert sum(len(set(p["op"][p["oj"] == j])) < (p["oj"] == j).sum() for j in np.unique(p["oj"])) == 2
    if name == "pose_order_reversed":
        assert all((np.diff(p["op"][p["oj"] == j]) < 0).all() for j in np.unique(p["oj"]))
    if name == "clamp":
        assert p["points0"][-1, 2] > 1.9e6 and (p["oj"] == len(p["points0"]) - 1).sum() == len(p["poses0"])


def test_plain_windows_cover_the_window_sizes():
    ks = {len(scene(n)[0]["poses0"]) for n in SCENES}
    assert {2, 5, 14} <= ks


def run_oracle(p, max_iterations):
    poses, pts, s = O.ba_solve(p["poses0"], p["points0"], p["op"], p["oj"], p["uv"], BP.F, BP.CX, BP.CY, max_iterations=max_iterations)
    return poses, pts, Summary(s["iterations"], s["successful"], s["termination"], s["initial_cost"], s["final_cost"])


@pytest.mark.parametrize("name", list(SCENES))
def test_oracle_matches_the_reference(name):
    """The CPU oracle under the comparisons and tolerances of the GPU tests: the tolerances are right before a GPU is involved."""
    compare_with_reference(name, run_oracle, "oracle " + name)
    if name in BADLY_STARTED:
        for k in range(2, 7):
            compare_costs_after(name, run_oracle, "oracle " + name, k)


def run_product_lm(p, max_iterations):
    poses, pts, s, _, _ = O.product_lm_over_oracle_passes(p["poses0"], p["points0"], p["op"], p["oj"], p["uv"], BP.F, BP.CX, BP.CY, max_iterations=max_iterations)
    return poses, pts, Summary(s.iterations, s.successful_steps, s.termination, s.initial_cost, s.final_cost)


@pytest.mark.parametrize("name", ["bad_k3", "parameter_tolerance", "optimum", "k2_cap_30"])
def test_product_step_control_matches_the_reference(name):
    """svo_lm_solve (host/lm.cpp: speculative linearisation, one exchange per iteration) over the oracle's passes, as tests/test_lm.py
    drives it: rejections with growing decrease factors, the parameter tolerance, the gradient tolerance at the start, the cap."""
    compare_with_reference(name, run_product_lm, "host step control " + name)


def test_write_the_spread_table():
    """SVO_WRITE_BA_REF_SPREADS=<file>: the table of tests/ba_ref.py's docstring, from this run."""
    rows = []
    for name in SCENES:
        p, mi = scene(name)
        rows.append("%-22s %2d poses %5d obs  one iteration: cost %.1e  poses %.1e  landmarks %.1e | %2d iterations: cost %.1e  residuals %.1e" % (
            name, len(p["poses0"]), len(p["op"]), R.spread(p, "cost", 1), R.spread(p, "poses", 1), R.spread(p, "points", 1),
            R.reference(p, mi)[2].iterations, R.spread(p, "cost", mi), R.spread(p, "residuals", mi)))
    assert len(rows) == len(SCENES)
    if os.environ.get("SVO_WRITE_BA_REF_SPREADS"):
        with open(os.environ["SVO_WRITE_BA_REF_SPREADS"], "w") as f:
            f.write("\n".join(rows) + "\n")


# -------------------------------------------------------------------------------------------------------- GPU tests
FORMS = ("host", "wide", "compact", "mfma", "atomics")


def accepts(name, form):
    """The MFMA linearisation takes one observation per (landmark, pose) (host/ba_layout.h); everything else takes every scene."""
    return not (form == "mfma" and name == "twice")


def run_gpu(ctx, form):
    """host: the host-driven loop; wide / compact: the one-launch device-resident solves; mfma / atomics: the bulk accumulation paths."""
    import stereo_vo_amd as S

    def run(p, max_iterations):
        kw = dict(max_landmarks=len(p["points0"]) + 8, max_observations=len(p["op"]) + 8, max_time_s=0.0, max_iterations=max_iterations)
        if form == "host":
            kw.update(device_lm=False)
        elif form in ("wide", "compact"):
            kw.update(device_lm=True, solve_form=form)
        else:
            kw.update(accumulation=form)
        ba = S.api.BA(ctx, max(len(p["poses0"]), 2), BP.F, BP.CX, BP.CY, **kw)
        try:
            ba.load_problem(p["poses0"], p["points0"], p["op"], p["oj"], p["uv"])
            s = ba.solve_problem()
            poses, pts = ba.read_problem()
            if form in ("wide", "compact"):  # the form asked for is the form that ran
                forms, gave_up = ba.solve_forms()
                assert gave_up == 0 and sum(forms) == 1 and forms[0] == (1 if form == "compact" else 0), (form, forms, gave_up)
        finally:
            ba.close()
        return poses, pts, Summary(s.iterations, s.successful_steps, s.termination, s.initial_cost, s.final_cost)
    return run


@pytest.mark.gpu
@pytest.mark.parametrize("name,form", [(n, f) for n in SCENES for f in FORMS if accepts(n, f)])
def test_hip_window_solve_matches_the_reference(ctx, name, form):
    """Every scene through every form that accepts it, against the reference only: after one LM iteration the costs, every free pose
    parameter and every observed landmark; after the whole solve the counts, the final cost and the residual vector at the returned
    state; the oldest pose and the unobserved landmarks untouched."""
    compare_with_reference(name, run_gpu(ctx, form), form + " " + name)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", BADLY_STARTED)
def test_hip_badly_started_solves_follow_the_reference_step_by_step(ctx, name, form):
    """The cost after 2 .. 6 iterations (one solve per k) of the badly started scenes: rejected steps, shrinking radii, reused
    diagonals."""
    for k in range(2, 7):
        compare_costs_after(name, run_gpu(ctx, form), form + " " + name, k)
