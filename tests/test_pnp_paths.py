"""a5 PnP-RANSAC on scenes that reach every decision, judged by an independent restatement (tests/pnp_ref.py).

`tests/test_pnp.py` compares the kernel with the oracle on mild random scenes; the oracle shares the kernel's structure, and
none of those scenes fails a factorisation, leaves a loop by its damping, flips a quaternion, meets a NaN, puts a point on the
threshold or relaunches on a cap next to the 12 hypotheses of the first launch.  Here the scenes are built for those
decisions, the restatement counts them, and both the oracle (CPU) and `svo_pnp_ransac` (GPU) must return its bytes."""
import ctypes as C
import functools

import numpy as np
import pytest

import pnp_ref as P

KF, KCX, KCY = 718.856, 607.1928, 185.2157
Z3 = np.zeros(3)
NEAR_R, NEAR_T = (0.002, 0.001, -0.003), (0.01, 0.0, -0.1)   # the guess of the ordinary scenes
POSE_R, POSE_T = (0.01, -0.03, 0.005), (0.05, -0.02, -0.8)   # and their pose


# ----------------------------------------------------------------------------------------------------------------- scenes
def rodrigues(rv, dtype=np.float64):
    """Plain libm Rodrigues (the generator's and the geometric check's; the declared conversions are the code under test)."""
    rv = np.asarray(rv, dtype)
    th = np.sqrt((rv * rv).sum())
    if th == 0:
        return np.eye(3, dtype=dtype)
    k = rv / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], dtype)
    return np.eye(3, dtype=dtype) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def project(X, rv, tv, f, cx, cy, dtype=np.float64):
    Xc = np.asarray(X, dtype) @ rodrigues(rv, dtype).T + np.asarray(tv, dtype)
    return np.stack([dtype(f) * Xc[:, 0] / Xc[:, 2] + dtype(cx), dtype(f) * Xc[:, 1] / Xc[:, 2] + dtype(cy)], 1)


def scene(X, uv, r0=Z3, t0=Z3, f=KF, cx=KCX, cy=KCY, iterations=100, reproj_err=8.0, confidence=0.99, truth=None):
    return dict(X=np.ascontiguousarray(X, np.float32), uv=np.ascontiguousarray(uv, np.float32), f=f, cx=cx, cy=cy,
                r0=np.asarray(r0, np.float64), t0=np.asarray(t0, np.float64), iterations=iterations, reproj_err=reproj_err,
                confidence=confidence, truth=truth)


def _spoil(rng, uv, out):
    k = int(out.sum())
    uv[out] += rng.uniform(20, 80, (k, 2)) * rng.choice([-1, 1], (k, 2))


def noisy(seed, n, rv=POSE_R, tv=POSE_T, noise=0.3, outliers=0.2, r0=NEAR_R, t0=NEAR_T, **kw):
    """n world points seen from the pose (rv, tv): pixels with Gaussian noise; `outliers` of them (a fraction, or a count taken
    from the end) are moved 20 to 80 px away."""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-8, 8, n), rng.uniform(-2, 2, n), rng.uniform(6, 40, n)], 1).astype(np.float32)
    uv = project(X, rv, tv, KF, KCX, KCY) + rng.normal(0, noise, (n, 2))
    _spoil(rng, uv, np.arange(n) >= n - outliers if isinstance(outliers, int) else rng.random(n) < outliers)
    return scene(X, uv, r0, t0, truth=(np.asarray(rv, float), np.asarray(tv, float)), **kw)


def camera_frame(seed, n, rv, tv, noise=0.2, outliers=0.2, dr=0.01):
    """The points are drawn in the CAMERA frame, in front of it, and carried back to the world, so that any rotation is a valid
    view; the guess is the pose turned by `dr` more about its own axis."""
    rng = np.random.default_rng(seed)
    Xc = np.stack([rng.uniform(-8, 8, n), rng.uniform(-2, 2, n), rng.uniform(6, 40, n)], 1)
    X = ((Xc - np.asarray(tv)) @ rodrigues(rv)).astype(np.float32)
    uv = project(X, rv, tv, KF, KCX, KCY) + rng.normal(0, noise, (n, 2))
    _spoil(rng, uv, rng.random(n) < outliers)
    rv = np.asarray(rv, float)
    return scene(X, uv, rv * (1 + dr / np.linalg.norm(rv)), tv, truth=(rv, np.asarray(tv, float)))


def depth_range(seed, n, noise, err, zlo, zhi, guess_scale):
    """Depths spread log-uniformly over [zlo, zhi] and heavy pixel noise under a wide threshold: a large-residual problem, on
    which the refinement converges slowly enough to reach the floor of its damping or its iteration cap."""
    rng = np.random.default_rng(seed)
    z = np.exp(rng.uniform(np.log(zlo), np.log(zhi), n))
    X = np.stack([rng.uniform(-0.6, 0.6, n) * z, rng.uniform(-0.2, 0.2, n) * z, z], 1).astype(np.float32)
    rv, tv = np.array([0.05, -0.1, 0.02]), np.array([0.3, -0.1, 0.2])
    uv = project(X, rv, tv, KF, KCX, KCY) + rng.normal(0, noise, (n, 2))
    return scene(X, uv, rv * guess_scale, tv * guess_scale, reproj_err=err, truth=(rv, tv))


LATTICE_N = 400
LATTICE_SPECIAL = ("ex_plus_err", "ey_minus_err", "just_outside", "mirrored", "outlier")
ERR_INEXACT = 1.0 + 2.0 ** -12  # exact in f32; its square 1 + 2^-11 + 2^-24 is exact in f64 and rounds down to 1 + 2^-11 in f32


def lattice(err, origin=None):
    """Exact arithmetic: f = 512, c = 256, zero guess (R = I exactly), X / Z and Y / Z on a 1/32 grid, Z in {2, 4, 8}: every pixel
    is exact in f32 and every residual exact in f64.  Hypothesis 0 samples five exact points, so it stays at the identity and
    leaves its loop by the damping.  With 400 points the cap falls to 1 after it.  Five other points (LATTICE_SPECIAL) sit on
    and around the threshold `err`, which is exact in f32.
    origin: instead of those five, one point AT the world origin under a guess whose translation is next to nothing, so that
    the point is an inlier of hypothesis 0 while its Jacobian is of the order 1e162 or 1e307:
      "chol"  t = (2.5e-161, 0, 1e-160), pixel (384, 256): H has +inf and -inf entries, every factorisation of the refinement
              fails and the refinement ends at its iteration cap;
      "nan"   t = (0, 0, 1e-305), pixel (250, 256), ex = 6: H[3][3] and g[3] are +inf, the factorisation succeeds, the step and
              with it the candidate's cost are NaN, and the refinement leaves by its damping.
    Either way the pose comes back untouched."""
    n = LATTICE_N
    i = np.arange(n)
    Z = np.array([2.0, 4.0, 8.0])[i % 3]
    X = ((i * 7) % 33 - 16) / 32.0 * Z
    Y = ((i * 5) % 29 - 14) / 32.0 * Z
    W = np.stack([X, Y, Z], 1)
    uv = np.stack([512 * X / Z + 256, 512 * Y / Z + 256], 1)
    keep, _ = P.draw(0, n)
    sp = [k for k in range(n) if k not in keep][3:8]
    if origin:
        W[sp[0]] = 0.0
        uv[sp[0]] = (384.0, 256.0) if origin == "chol" else (250.0, 256.0)
        t0 = (2.5e-161, 0.0, 1e-160) if origin == "chol" else (0.0, 0.0, 1e-305)
        return scene(W, uv, t0=t0, f=512.0, cx=256.0, cy=256.0, reproj_err=err)
    uv[sp[0], 0] -= err               # ex = +err exactly
    uv[sp[1], 1] += err               # ey = -err exactly
    uv[sp[2], 0] -= err + 2.0 ** -8   # ex = err + 2^-8
    W[sp[3]] = -W[sp[3]]              # the same pixel from behind the camera
    uv[sp[4]] += (50.0, -37.0)
    s = scene(W, uv, f=512.0, cx=256.0, cy=256.0, reproj_err=err)
    assert np.array_equal(s["X"].astype(np.float64), W) and np.array_equal(s["uv"].astype(np.float64), uv)  # exact in f32
    s["special"] = dict(zip(LATTICE_SPECIAL, sp))
    return s


def _hostile(seed, n):
    s = noisy(seed, n, (0.01, -0.02, 0.005), (0.05, -0.02, -0.4), outliers=0.1, r0=Z3, t0=Z3)
    s["truth"] = None
    return s


@functools.lru_cache(maxsize=None)
def scenes():
    S = {"lattice_8": lattice(8.0), "lattice_inexact": lattice(ERR_INEXACT), "origin_chol": lattice(8.0, "chol"),
         "origin_nan": lattice(8.0, "nan")}
    for th in (3.0, 3.3, 6.0):  # |rvec| / 2 beyond pi / 2 starts at w < 0
        S["rot_%g" % th] = camera_frame(20, 500, (0.0, th, 0.0), (0.3, -0.1, 0.5))
    s = _hostile(31, 64)
    s["X"][::9, 2] = 0.0
    S["camera_plane"] = s
    s = _hostile(32, 140)
    s["X"][::7] = np.nan
    S["nan_points"] = s
    s = _hostile(33, 100)
    s["X"] *= np.float32(1e30)
    S["huge"] = s
    X = np.tile(np.array([[1.0, -0.5, 10.0]]), (40, 1))
    S["coincident"] = scene(X, project(X, (0.02, 0.01, 0.0), (0.1, 0.0, 0.2), KF, KCX, KCY))
    X = np.array([[0.0, 0.0, 12.0]]) + np.linspace(-1, 1, 80)[:, None] * np.array([[4.0, 1.0, 3.0]])
    S["collinear"] = scene(X, project(X, (0.02, 0.01, 0.0), (0.1, 0.0, 0.2), KF, KCX, KCY))
    rng = np.random.default_rng(34)
    X = np.stack([rng.uniform(-10, 10, 300), rng.uniform(-3, 3, 300), rng.uniform(-20, 20, 300)], 1)
    rv, tv = np.array([0.0, 0.1, 0.0]), np.array([0.2, 0.0, 1.0])
    uv = project(X, rv, tv, KF, KCX, KCY) + rng.normal(0, 0.3, (300, 2))
    S["around_camera"] = scene(X, uv, rv + (0.0, 0.4, 0.0), tv + (2.0, 0.0, -2.2))
    S["at_guess_exact"] = noisy(35, 200, Z3, Z3, noise=0.0, outliers=0.1, r0=Z3, t0=Z3)
    S["at_guess_1e-4"] = noisy(35, 200, Z3, Z3, noise=1e-4, outliers=0.1, r0=Z3, t0=Z3)
    S["far_guess_a"] = noisy(36, 300, (0.3, -0.4, 0.1), (2.0, -1.0, 2.0), r0=Z3, t0=Z3)
    S["far_guess_b"] = noisy(37, 300, (-0.5, 0.5, 0.3), (-3.0, 1.0, 3.5), r0=Z3, t0=Z3)
    for it in (1, 4, 11, 12, 13, 100):
        S["shape_it%d" % it] = noisy(38, 500, outliers=0.3, iterations=it)
    S["err_0.5"] = noisy(39, 400, outliers=0.3, reproj_err=0.5)
    S["conf_1"] = noisy(40, 200, confidence=1.0)
    S["conf_0"] = noisy(40, 200, confidence=0.0)
    for n in (5, 6, 63, 64, 65, 128, 129, 257):  # the 64-bit words of the inlier masks
        S["n_%d" % n] = noisy(41 + n, n, outliers=0.15 if n > 6 else 0.0)
    for m in TREE_COUNTS:  # the levels of the refinement's tree
        S["inl_%d" % m] = noisy(300 + m, m + 12, noise=0.05, outliers=12)
    S["slow_floor"] = depth_range(1, 120, 50.0, 300.0, 0.3, 300.0, 0.0)
    S["slow_cap"] = depth_range(3, 120, 50.0, 300.0, 2.0, 20.0, 3.0)
    S["no_model"] = noisy(3, 60, outliers=1.0, r0=(0.3, -0.2, 0.1), t0=(1.0, 2.0, 3.0), reproj_err=0.05)
    for s in S.values():  # built once, shared by every test
        for k in ("X", "uv", "r0", "t0"):
            s[k].setflags(write=False)
    return S


TREE_COUNTS = (63, 64, 65, 127, 128, 129, 255, 256, 257)
SCENE_NAMES = ("lattice_8", "lattice_inexact", "origin_chol", "origin_nan", "rot_3", "rot_3.3", "rot_6", "camera_plane", "nan_points", "huge",
               "coincident", "collinear", "around_camera", "at_guess_exact", "at_guess_1e-4", "far_guess_a", "far_guess_b",
               "shape_it1", "shape_it4", "shape_it11", "shape_it12", "shape_it13", "shape_it100", "err_0.5", "conf_1", "conf_0",
               "n_5", "n_6", "n_63", "n_64", "n_65", "n_128", "n_129", "n_257") + tuple("inl_%d" % m for m in TREE_COUNTS) + (
               "slow_floor", "slow_cap", "no_model")


def _args(s):
    return (s["X"], s["uv"], s["f"], s["cx"], s["cy"], s["r0"], s["t0"], s["iterations"], s["reproj_err"], s["confidence"])


@functools.lru_cache(maxsize=None)
def ref(name, variant=None):
    """The restatement's answer on a scene, computed once and shared (read-only)."""
    r, t, inl, rec = P.pnp_ransac(*_args(scenes()[name]), variant=variant)
    for a in (r, t, inl):
        a.setflags(write=False)
    return r, t, inl, rec


def _same(got, want):
    return (np.array_equal(got[2], want[2]) and np.array_equal(got[0], want[0], equal_nan=True)
            and np.array_equal(got[1], want[1], equal_nan=True))


def _counter(name, path):
    rec = ref(name)[3]
    stage, _, key = path.rpartition(".")
    return rec[stage][key] if stage else rec[key]


# -------------------------------------------------------------------------------------------------------------- CPU tests
def test_scene_list_is_complete_and_small():
    S = scenes()
    assert tuple(S) == SCENE_NAMES
    assert max(len(s["X"]) for s in S.values()) <= 2000


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_oracle_returns_the_restatements_bytes(name):
    import oracle_lib as O
    got = O.pnp_ransac(*_args(scenes()[name]))
    want = ref(name)
    assert np.array_equal(got[2], want[2])
    assert np.array_equal(got[0], want[0], equal_nan=True) and np.array_equal(got[1], want[1], equal_nan=True), (got[:2], want[:2])


def test_declared_functions_equal_the_oracles_taps_bit_for_bit():
    import oracle_lib as O
    rng = np.random.default_rng(5)
    xs = np.concatenate([rng.uniform(1e-300, 1.0, 1500), 10.0 ** rng.uniform(-300, 0, 1500), [1.0, 0.5, 0.01, 2.2250738585072014e-308,
                         0.70710678118654757, 0.70710678118654746]])
    for x in xs.tolist():
        assert P.det_log(x) == O.pnp_det_log(x), x
    for n in (5, 6, 7, 64, 300, 731, 2000):
        for cnt in range(5, n + 1, max(1, n // 61)):
            for conf in (0.99, 0.5, 0.0, 1.0):
                for mx in (100, 37, 13, 12, 3):
                    ep = (n - cnt) / n
                    assert P.update_num_iters(conf, ep, 5, mx) == O.pnp_update_num_iters(conf, ep, 5, mx), (n, cnt, conf, mx)
    for x in rng.uniform(0, 7.0, 3000).tolist() + [0.0, 1e-9, 0.5, 0.5000000001, 1.0, np.pi / 2, np.pi, 2 * np.pi]:
        assert P.det_sincos(x) == O.det_sincos(x), x
    pts = [(1.0, 1.0), (0.0, 1.0), (1.0, 0.0), (1e-12, 1.0), (1.0, 1e-12), (0.41421356237309503, 1.0), (0.4142135623730951, 1.0),
           (1e-300, 1e-300)]
    pts += [tuple(v) for v in rng.uniform(0, 1, (3000, 2)).tolist()]
    pts += list(zip((10.0 ** rng.uniform(-12, 0, 500)).tolist(), (10.0 ** rng.uniform(-12, 0, 500)).tolist()))
    for y, x in pts:
        assert P.atan2_q1(y, x) == O.det_atan2_q1(y, x), (y, x)
    for k in range(2000):
        rv = rng.normal(size=3) * (1e-14, 1e-3, 0.3, 1.0, 2.5, 4.0)[k % 6]  # both small-angle branches and the flip beyond pi
        q, back = P.rvec_quat_roundtrip(rv)
        qo, backo = O.det_rvec_quat_roundtrip(rv)
        assert np.array_equal(q, qo) and np.array_equal(back, backo), rv


# What each scene is for: counters of the restatement, exact.  "min." is the 5-point solve (summed over the hypotheses
# consumed), "ref." the refinement, the rest belongs to the call.
EXPECT = {
    "lattice_8": {"min.accept": 0, "min.reject": 10, "min.exit_lambda": 1, "z_le_0": 1},
    "lattice_inexact": {"min.accept": 0, "min.reject": 10, "min.exit_lambda": 1, "z_le_0": 1},
    "origin_chol": {"ref.chol_fail": 20, "ref.exit_cap": 1, "ref.accept": 0, "ref.reject": 0},
    "origin_nan": {"ref.chol_fail": 0, "ref.nan_cost": 10, "ref.reject": 10, "ref.exit_lambda": 1},
    "rot_3": {"quat_flip": 0}, "rot_3.3": {"quat_flip": 1}, "rot_6": {"quat_flip": 1},
    "camera_plane": {"min.chol_fail": 96, "z_le_0": 138},
    "nan_points": {"min.chol_fail": 108, "min.nan_cost": 9, "z_le_0": 320},
    "huge": {"min.accept": 97, "ref.accept": 5, "ref.reject": 5},
    "coincident": {"ref.accept": 1, "ref.exit_abs": 1},
    "collinear": {"ref.accept": 4, "ref.exit_rel": 1},
    "around_camera": {"z_le_0": 13269, "min.exit_cap": 46},
    "at_guess_exact": {"min.exit_abs_alone": 3, "ref.exit_abs_alone": 1},
    "at_guess_1e-4": {"min.exit_abs_alone": 1, "ref.exit_abs": 1, "ref.exit_abs_alone": 0},
    "far_guess_a": {"min.lam_floor": 18, "min.exit_cap": 2},
    "far_guess_b": {"min.lam_floor": 14, "min.exit_cap": 1},
    "conf_1": {"tie": 20},
    "n_5": {"dup_draw": 3, "ref.reject": 10, "ref.exit_lambda": 1},
    "n_6": {"dup_draw": 1, "min.exit_cap": 1},
    "slow_floor": {"ref.accept": 8, "ref.lam_floor": 2, "ref.exit_rel": 1},
    "slow_cap": {"ref.accept": 6, "ref.reject": 14, "ref.exit_cap": 1},
    "no_model": {"min.exit_cap": 35, "dup_draw": 16},
}
LM_MANDATORY_BOTH = ("accept", "reject", "nan_cost", "exit_abs", "exit_abs_alone", "exit_rel", "exit_lambda")
LM_MANDATORY_MIN = ("exit_cap", "chol_fail", "lam_floor")
NOT_REACHED = ()  # of ref.chol_fail, ref.exit_cap, ref.lam_floor: all three are reached (origin_chol, slow_cap, slow_floor)


def test_every_scene_reaches_what_it_was_built_for():
    got = {name: {path: _counter(name, path) for path in want} for name, want in EXPECT.items()}
    assert got == EXPECT


def test_every_decision_is_reached_on_some_scene():
    total = {}
    for name in SCENE_NAMES:
        rec = ref(name)[3]
        for key in P.CALL_COUNTERS:
            total[key] = total.get(key, 0) + rec[key]
        for stage in ("min", "ref"):
            for key in P.LM_COUNTERS:
                total[stage + "." + key] = total.get(stage + "." + key, 0) + rec[stage][key]
    assert set(NOT_REACHED) <= {"ref.chol_fail", "ref.exit_cap", "ref.lam_floor"}
    assert tuple(sorted(k for k, v in total.items() if v == 0)) == tuple(sorted(NOT_REACHED)), total
    for key in LM_MANDATORY_BOTH:
        assert total["min." + key] > 0 and total["ref." + key] > 0, key
    for key in LM_MANDATORY_MIN + P.CALL_COUNTERS:
        assert total.get("min." + key, total.get(key)) > 0, key


def test_lattice_points_on_the_threshold():
    """ex = +err and ey = -err are inliers (<=), err + 2^-8 is not, the mirrored point is not (z < 0); a strict comparison
    loses both threshold points at either threshold, a threshold squared in f32 only where that square is inexact; without
    the z test the mirrored point, whose error is 0, comes in."""
    for name, f32sq_differs in (("lattice_8", False), ("lattice_inexact", True)):
        sp = scenes()[name]["special"]

        def inside(variant=None):
            r, t, inl, rec = ref(name, variant)
            assert rec["best"] == 0 and rec["counts"][0] == len(inl)
            assert variant is not None or (rec["niters"] == 1 and rec["min"]["exit_lambda"] == 1 and rec["min"]["accept"] == 0)
            others = np.setdiff1d(np.arange(LATTICE_N), list(sp.values()))
            assert np.isin(others, inl).all()
            return {k for k, i in sp.items() if i in inl}
        assert inside() == {"ex_plus_err", "ey_minus_err"}
        assert inside("thr_strict") == set()
        assert inside("thr_f32sq") == (set() if f32sq_differs else {"ex_plus_err", "ey_minus_err"})
        assert inside("no_z_test") == {"ex_plus_err", "ey_minus_err", "mirrored"}
    e = np.float32(ERR_INEXACT)
    assert float(e) == ERR_INEXACT and float(e * e) < float(e) * float(e) == 1 + 2.0 ** -11 + 2.0 ** -24


def test_scene_classes():
    rec = {name: ref(name)[3] for name in SCENE_NAMES}
    n_in = {name: len(ref(name)[2]) for name in SCENE_NAMES}
    # the cap lands exactly on the first launch's 12 hypotheses: nothing is relaunched, and nothing may be
    assert [name for name in SCENE_NAMES if rec[name]["niters"] == 12 and scenes()[name]["iterations"] == 100] == CAP_EXACTLY_12
    # the cap stays above 12: the call launches a second time
    assert [name for name in SCENE_NAMES if 13 <= rec[name]["niters"] <= 100 and scenes()[name]["iterations"] > 12] == RELAUNCHED
    assert rec["shape_it13"]["niters"] == 13 and rec["rot_3"]["niters"] == 13  # one above the first launch
    assert {name: rec[name]["best"] for name in SCENE_NAMES if rec[name]["best"] >= 12} == BEST_BEYOND_FIRST_LAUNCH
    assert [name for name in SCENE_NAMES if rec[name]["best"] < 0] == ["no_model"] and n_in["no_model"] == 0
    assert np.array_equal(ref("no_model")[0], scenes()["no_model"]["r0"]) and np.array_equal(ref("no_model")[1], scenes()["no_model"]["t0"])
    assert np.isnan(scenes()["nan_points"]["X"]).any(axis=1).sum() == 20  # and none of them is ever an inlier
    assert all(np.isfinite(scenes()[name]["X"][ref(name)[2]]).all() for name in SCENE_NAMES)
    assert rec["conf_1"]["niters"] == 100 and len(rec["conf_1"]["counts"]) == 100
    assert rec["conf_0"]["niters"] == 0 and len(rec["conf_0"]["counts"]) == rec["conf_0"]["best"] + 1
    assert rec["n_5"]["dup_draw"] > 0 and rec["n_6"]["dup_draw"] > 0 and sum(r["tie"] for r in rec.values()) > 0
    assert [n_in["inl_%d" % m] for m in TREE_COUNTS] == list(TREE_COUNTS)
    assert [len(rec["shape_it%d" % it]["counts"]) for it in (1, 4, 11, 12, 13, 100)] == [1, 4, 11, 12, 13, rec["shape_it100"]["niters"]]
    for name in ("rot_3", "rot_3.3", "rot_6"):
        assert rec[name]["quat_flip"] == (0 if name == "rot_3" else 1)
        assert abs(np.linalg.norm(ref(name)[0]) - (2 * np.pi - np.linalg.norm(scenes()[name]["truth"][0])
                                                   if rec[name]["quat_flip"] else np.linalg.norm(scenes()[name]["truth"][0]))) < 1e-3


CAP_EXACTLY_12 = ["n_63", "n_65"]
RELAUNCHED = ["rot_3", "rot_3.3", "rot_6", "camera_plane", "nan_points", "huge", "around_camera", "shape_it13", "shape_it100", "err_0.5",
              "conf_1", "no_model"]
BEST_BEYOND_FIRST_LAUNCH = {"around_camera": 52, "err_0.5": 76}

# variant -> the scenes, of these, whose returned bytes (inliers, rvec, tvec) it changes.  VARIANT_SCENES is a subset of
# SCENE_NAMES chosen for run time (ten variants over all scenes would take several times as long), one or two scenes of each
# kind; the map is exact over this subset and says nothing about the scenes left out (huge, collinear, err_0.5, ...).
VARIANT_SCENES = ("lattice_8", "lattice_inexact", "rot_3.3", "camera_plane", "nan_points", "coincident", "around_camera", "at_guess_exact",
                  "at_guess_1e-4", "far_guess_a", "shape_it13", "conf_0", "n_5", "n_6", "n_64", "inl_128", "inl_257", "slow_floor", "slow_cap")
VARIANT_CHANGES = {
    "tie_replaces": ("rot_3.3", "camera_plane", "nan_points", "at_guess_exact", "at_guess_1e-4", "far_guess_a", "shape_it13", "n_64", "inl_128"),
    "thr_strict": ("lattice_8", "lattice_inexact"),
    "thr_f32sq": ("lattice_inexact",),
    "no_z_test": ("lattice_8", "lattice_inexact", "around_camera"),
    "seq_sum": ("lattice_8", "lattice_inexact", "rot_3.3", "camera_plane", "nan_points", "around_camera", "at_guess_exact", "at_guess_1e-4",
                "far_guess_a", "shape_it13", "conf_0", "n_6", "n_64", "inl_128", "inl_257", "slow_floor", "slow_cap"),
    "min_tree": ("rot_3.3", "camera_plane", "nan_points", "coincident", "around_camera", "at_guess_exact", "at_guess_1e-4", "far_guess_a",
                 "shape_it13", "conf_0", "n_5", "n_6", "n_64", "inl_128", "inl_257", "slow_floor", "slow_cap"),
    "no_jitter": ("rot_3.3", "camera_plane", "nan_points", "coincident", "at_guess_exact", "at_guess_1e-4", "far_guess_a", "shape_it13",
                  "conf_0", "n_5", "n_6", "n_64", "inl_128", "inl_257", "slow_cap"),
    "no_lam_floor": ("slow_floor", "slow_cap"),
    "no_cap": ("lattice_8", "lattice_inexact", "around_camera", "slow_floor", "slow_cap"),
    "no_abs_stop": ("at_guess_exact",),
}


def test_every_misreading_changes_some_scenes_bytes():
    got = {v: tuple(name for name in VARIANT_SCENES if not _same(ref(name, v), ref(name))) for v in P.VARIANTS}
    assert all(got.values())
    assert got == VARIANT_CHANGES, got


# ------------------------------------------------------------------------------------------- the tolerance-free check
# Scenes generated from a known pose with pixel noise.  The refinement minimises the reprojection cost over the returned
# inliers, so that cost at the returned pose must not exceed the cost at the pose the scene was generated from.
GEOMETRIC = tuple(name for name in SCENE_NAMES if name.startswith(("rot_", "far_guess", "shape_it", "err_", "conf_", "n_", "inl_", "slow_"))
                  or name == "at_guess_1e-4")
# not used: at_guess_exact (noise 0: the cost at the true pose is the f32 rounding of the pixels alone, and both costs are
# rounding noise); the hostile scenes have no pose.


def _cost_ld(s, rv, tv, inl):
    LD = np.longdouble
    e = project(s["X"][inl], rv, tv, LD(np.float32(s["f"])), LD(np.float32(s["cx"])), LD(np.float32(s["cy"])), LD) - s["uv"][inl].astype(LD)
    return (e * e).sum()


def _geometric(name, r, t, inl):
    s = scenes()[name]
    assert len(inl) >= 5
    got, true = _cost_ld(s, r, t, inl), _cost_ld(s, *s["truth"], inl)
    assert got <= true, (name, got, true)


@pytest.mark.parametrize("name", GEOMETRIC)
def test_restatement_beats_the_true_pose_on_its_own_inliers(name):
    assert len(GEOMETRIC) >= 8
    _geometric(name, *ref(name)[:3])


# -------------------------------------------------------------------------------------------------------------- GPU tests
def _gpu(ctx, name):
    return ctx.pnp_ransac(*_args(scenes()[name]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_hip_returns_the_restatements_bytes(ctx, name):
    """svo_pnp_ransac against the restatement (not the oracle): the inlier list and the pose with ==.  tests/test_pnp.py
    allows the pose 1e-12 absolute; on an MI355X every scene here had rvec and tvec equal bit for bit (largest difference
    0.0), so the stricter of the two rules is the one kept."""
    r, t, inl = _gpu(ctx, name)
    rw, tw, iw, _ = ref(name)
    assert np.array_equal(inl, iw)
    assert np.isfinite(scenes()[name]["X"][inl]).all()  # a NaN point is never an inlier, whatever the restatement says
    assert np.array_equal(r, rw, equal_nan=True) and np.array_equal(t, tw, equal_nan=True), (np.abs(r - rw).max(), np.abs(t - tw).max())


@pytest.mark.gpu
def test_hip_result_does_not_depend_on_the_calls_before_it(ctx):
    """One context reuses its scratch: hypothesis counts, masks and the arrival counter of a larger or longer call lie under
    the next one.  Large n then n = 5; 100 hypotheses then 1; a relaunching call then a one-launch call; no model then a
    model; and the first scene again."""
    order = ("shape_it100", "n_5", "conf_1", "shape_it1", "rot_3", "conf_0", "no_model", "far_guess_a", "shape_it100")
    assert ref("rot_3")[3]["niters"] > 12 >= len(ref("conf_0")[3]["counts"]) and ref("no_model")[3]["best"] < 0
    for name in order:
        assert _same(_gpu(ctx, name), ref(name)), name


def _raw(ctx, X, uv, n, rv, tv, iterations, inl, m):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return ctx.L.svo_pnp_ransac(ctx.h, p(X), p(uv), n, C.c_float(KF), C.c_float(KCX), C.c_float(KCY), p(rv), p(tv), iterations,
                                C.c_float(8.0), C.c_double(0.99), p(inl), None if m is None else C.byref(m))


@pytest.mark.gpu
def test_hip_refusals_and_empty_inputs_leave_the_pose_alone(ctx):
    """Through the C entry: iterations outside 1..1024 and a null rvec3 / n_inliers are SVO_ERR_INVALID; n = 0 (with null
    arrays) and n = 4 are SVO_OK with no inliers; none of them touches the pose, and the next ordinary call is right."""
    s = scenes()["n_64"]
    X, uv = s["X"], s["uv"]
    INVALID, OK = -1, 0
    cases = (("iterations 0", dict(iterations=0), INVALID), ("iterations 1025", dict(iterations=1025), INVALID),
             ("null rvec3", dict(rv=None), INVALID), ("null n_inliers", dict(m=None), INVALID),
             ("n 0", dict(n=0, X=None, uv=None, inl=None), OK), ("n 4", dict(n=4), OK))
    for what, change, status in cases:
        rv, tv = np.array([0.3, -0.2, 0.1]), np.array([1.0, 2.0, 3.0])
        a = dict(X=X, uv=uv, n=len(X), rv=rv, tv=tv, iterations=100, inl=np.full(len(X), -7, np.int32), m=C.c_int(-7))
        a.update(change)
        assert _raw(ctx, **a) == status, what
        assert np.array_equal(rv, [0.3, -0.2, 0.1]) and np.array_equal(tv, [1.0, 2.0, 3.0]), what
        if a["m"] is not None:  # a refusal touches nothing: the count keeps its sentinel
            assert a["m"].value == (0 if status == OK else -7), what
        if a["inl"] is not None:
            assert (a["inl"] == -7).all(), what
        assert _same(_gpu(ctx, "n_64"), ref("n_64")), what


@pytest.mark.gpu
@pytest.mark.parametrize("name", GEOMETRIC)
def test_hip_beats_the_true_pose_on_its_own_inliers(ctx, name):
    _geometric(name, *_gpu(ctx, name))
