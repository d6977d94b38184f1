"""Keyframe geometry (a6 dedup, a8 triangulation) against an independent whole-array restatement (tests/geom_ref.py), on inputs that
are BUILT to reach every decision and every launch-shape edge, and the fused forms the pipelines run against the composition
corner_detect -> geom_ref.dedup -> stereo_bm > 0.  Every comparison is == on bytes.

Inputs (named functions, fixed seeds; the counters of the restatement are literals below, generated once on the CPU):
  thr_30, thr_10.1, thr_7, thr_1   dedup threshold pairs: integer detected pixels, one f32 tracked point on the circle of radius min_d
                                   +- 2e-5 around each, found by a seeded search for the pairs a misreading decides differently
  shape cases                      n_det x n_trk at the edges of the 4-corner workgroup and of the 64-lane tracked loop, designed hits
  dd_zero, dd_negative, dd_huge    min_d = 0, min_d < 0, coordinates of 3e19 (dx * dx = +inf)
  mask cases                       keep masks against CT = 1024 and the 64-lane wave
  val_<pose>_<camera>              disparities k/16 and the specials -1, +0, -0, 1.4e-45, 2^-126, NaN; three poses, two cameras
  tri_specials                     the specials with +inf added (its outputs are NaN: inf / inf; compared as "NaN at the same places",
                                   payload bits are not part of the contract)"""
import ctypes as C
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

import geom_ref as GR
import oracle_lib as O

gpu = pytest.mark.gpu
F = np.float32
KITTI = (718.856, 607.1928, 185.2157, 0.537165718864418)
SMALL = (385.7545, 323.1205, 236.7432, 0.05)
CAMERAS = {"kitti": KITTI, "small": SMALL}


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ================================================================================================ dedup inputs
THRESHOLDS = {"thr_30": (30.0, 301), "thr_10.1": (10.1, 302), "thr_7": (7.0, 303), "thr_1": (1.0, 304)}
PER_SIDE = 30      # pairs taken per variant and outcome (kept / dropped)
PER_EDGE = 60      # pairs taken with distance == min_d, and with distance one ulp below
CANDIDATES = 3000000


def _pairwise(x, y, tx, ty, min_d, variant=None):
    return GR._hit_plane(x, y, tx, ty, min_d, variant)


@functools.lru_cache(maxsize=None)
def threshold_input(name):
    """One detected integer pixel per cell of a 40 x 40 lattice (pitch 3 min_d + 8: a tracked point is nearer than 1.25 min_d to its own
    detected pixel only, so every decision is that of one pair), its tracked point at distance min_d +- 2e-5 in a random direction.  Of
    3,000,000 seeded candidates the first PER_SIDE per variant and outcome that the variant decides differently are taken, the first
    PER_EDGE whose f32 distance is min_d itself and one ulp below it, and 40 plain ones (20 at 0.5 min_d, 20 at 1.2 min_d)."""
    min_d, seed = THRESHOLDS[name]
    rng = np.random.default_rng(seed)
    m = F(min_d)
    pitch = int(math.ceil(3 * min_d)) + 8
    n = CANDIDATES
    det = np.stack([rng.integers(0, 40, n) * pitch + pitch // 2 + rng.integers(-2, 3, n),
                    rng.integers(0, 40, n) * pitch + pitch // 2 + rng.integers(-2, 3, n)], 1).astype(F)
    th = rng.uniform(0, 2 * np.pi, n)
    r = float(m) + rng.uniform(-2e-5, 2e-5, n)
    r[:20] = 0.5 * float(m)
    r[20:40] = 1.2 * float(m)
    trk = (det.astype(np.float64) + np.stack([r * np.cos(th), r * np.sin(th)], 1)).astype(F)
    dist, hit = _pairwise(det[:, 0], det[:, 1], trk[:, 0], trk[:, 1], m)
    cell = (det[:, 0] // pitch).astype(int) * 40 + (det[:, 1] // pitch).astype(int)
    used, idx = set(), []

    def take(candidates, quota):  # the first `quota` candidates whose lattice cell is still free
        for k in candidates:
            if quota and cell[k] not in used:
                used.add(cell[k])
                idx.append(k)
                quota -= 1

    take(range(40), 40)
    for v in GR.DEDUP_VARIANTS:
        flip = _pairwise(det[:, 0], det[:, 1], trk[:, 0], trk[:, 1], m, v)[1] != hit
        for outcome in (False, True):
            take(np.flatnonzero(flip & (hit == outcome)), PER_SIDE)
    take(np.flatnonzero(dist == m), PER_EDGE)
    take(np.flatnonzero(dist == np.nextafter(m, F(-np.inf))), PER_EDGE)
    idx = np.array(idx)
    det, trk = det[idx], trk[idx]
    det, trk = det[rng.permutation(len(det))], trk[rng.permutation(len(trk))]
    assert (det == np.round(det)).all()
    return _ro(np.ascontiguousarray(det), np.ascontiguousarray(trk)) + (float(min_d),)


N_DET = (1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025)
N_TRK = (0, 1, 63, 64, 65, 127, 128, 129)
PATTERNS = ("trk_last", "trk_first", "trk_64", "det_last", "det_first", "all", "none")


def shape_pairs():
    """Every n_det with three n_trk; the 33 consecutive indices give every n_trk four or five n_det."""
    return [(nd, N_TRK[(3 * i + k) % len(N_TRK)]) for i, nd in enumerate(N_DET) for k in range(3)]


def shape_input(nd, nt, pattern):
    """(det, trk, min_d, expected kept mask) or None where the pattern does not exist at this shape.

    Private layout (all but "all"): detected pixel i on a lattice of pitch 100, tracked point j 2,000 px away from all of them unless it
    is the designed hit, which lies (5.5, -3.25) from its detected pixel; min_d = 30.  "all": detected pixel i belongs to cluster
    i mod n_trk, a block of at most 33 x 33 integer pixels round tracked point i mod n_trk (pitch 200, min_d = 40 > 17 sqrt 2): every
    detected pixel is dropped, by exactly one tracked point, and the tracked index that drops it runs over all lanes and chunks."""
    i = np.arange(nd)
    j = np.arange(nt)
    if pattern == "all":
        if nt == 0:
            return None
        c, k = i % nt, i // nt
        centre = np.stack([200 * (j % 12) + 100, 200 * (j // 12) + 100], 1).astype(F)
        det = (centre[c] + np.stack([k % 33 - 16, k // 33 - 16], 1)).astype(F)
        return det, centre + F(0.25), 40.0, np.zeros(nd, bool)
    det = np.stack([100 * (i % 40) + 3, 100 * (i // 40) + 7], 1).astype(F)
    trk = np.stack([-2000.5 - 10 * j, np.full(nt, -2000.25)], 1).astype(F)
    keep = np.ones(nd, bool)
    if pattern != "none":
        if nt == 0 or (pattern == "trk_64" and nt < 65):
            return None
        jt = {"trk_last": nt - 1, "trk_first": 0, "trk_64": 64, "det_last": nt // 2, "det_first": nt // 2}[pattern]
        it = {"trk_last": nd // 2, "trk_first": nd // 2, "trk_64": nd // 2, "det_last": nd - 1, "det_first": 0}[pattern]
        trk[jt] = det[it] + np.array([5.5, -3.25], F)
        keep[it] = False
    return det, trk, 30.0, keep


def shape_cases():
    out = []
    for nd, nt in shape_pairs():
        for p in PATTERNS:
            c = shape_input(nd, nt, p)
            if c is not None:
                out.append(("%s_%dx%d" % (p, nd, nt),) + c)
    return out


def special_dedup_inputs():
    """dd_zero / dd_negative: 70 detected pixels, every second one with a tracked point exactly on it (distance 0: not < 0, kept) and the
    others with one 3 px away; min_d = 0 and -1 keep everything (sqrt >= 0).  dd_huge: coordinates of 3e19 on opposite sides, dx * dx
    overflows to +inf, inf < 30 is false: kept; two ordinary pixels, one of them dropped, ride along."""
    i = np.arange(70)
    det = np.stack([17 * i + 5, 11 * (i % 9) + 40], 1).astype(F)
    trk = det.copy()
    trk[1::2] += np.array([3.0, 0.0], F)
    big = F(3e19)
    det_h = np.array([[big, 0], [0, big], [-big, -big], [100, 100], [300, 100]], F)
    trk_h = np.array([[-big, 0], [0, -big], [big, big], [110, 100], [-big, 100]], F)
    return {"dd_zero": (det, trk, 0.0, np.ones(70, bool)), "dd_negative": (det, trk, -1.0, np.ones(70, bool)),
            "dd_huge": (det_h, trk_h, 30.0, np.array([1, 1, 1, 0, 1], bool))}


# ================================================================================================ triangulation inputs
POSES = {
    "identity": np.eye(4, dtype=F),
    "rotated": np.array([[0.9998, -0.01, 0.02, 0.3], [0.01, 0.9999, 0.003, -0.1], [-0.02, -0.003, 0.9998, 2.5], [0, 0, 0, 1]], F),
    "far": np.array([[0.9998, -0.01, 0.02, 1e3], [0.01, 0.9999, 0.003, -1e3], [-0.02, -0.003, 0.9998, 1e3], [0, 0, 0, 1]], F),
}
SPECIALS = np.array([-1.0, 0.0, -0.0, 1.4e-45, 2.0 ** -126, np.nan], F)
TRI_N = (1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3073)
MASK_N = (65, 1023, 1024, 1025, 2047, 2048, 2049, 3073)
MASKS = ("first", "last", "alternate_lanes", "alternate_waves", "chunk0_empty", "chunk0_only", "one_per_chunk_last_lane")


def keep_mask(n, kind):
    i = np.arange(n)
    return {"all": np.ones(n, bool), "none": np.zeros(n, bool), "first": i == 0, "last": i == n - 1,
            "alternate_lanes": i % 2 == 1, "alternate_waves": (i // 64) % 2 == 0,
            "chunk0_empty": (i >= 1024) & (i < 2048), "chunk0_only": i < 1024,
            "one_per_chunk_last_lane": (i % 1024 == 1023) | (i == n - 1)}[kind]


def mask_cases():
    return [(n, k) for n in TRI_N for k in ("all", "none")] + [(n, k) for k in MASKS for n in MASK_N]


@functools.lru_cache(maxsize=None)
def mask_input(n, kind):
    """xy uniform over a KITTI frame, kept disparities from k/16, dropped ones -1, -1, 0, 0, ... by index; the rotated pose."""
    rng = np.random.default_rng(1000 + n)
    xy = (rng.uniform(0, 1, (n, 2)) * [1241, 376]).astype(F)
    keep = keep_mask(n, kind)
    disp = np.where(keep, rng.integers(1, 768, n) / 16.0, np.where(np.arange(n) % 4 < 2, -1.0, 0.0)).astype(F)
    return _ro(xy, disp, keep)


@functools.lru_cache(maxsize=None)
def value_input(pose, cam):
    """1,500 features: 1,200 disparities k/16 (1 <= k < 768), 50 of each special (no +inf: with an affine pose its w is inf and
    inf / inf is NaN), shuffled; integer and sub-pixel positions alternate (detector / tracker)."""
    rng = np.random.default_rng(sorted(POSES).index(pose) * 10 + sorted(CAMERAS).index(cam) + 500)
    n = 1500
    disp = np.concatenate([rng.integers(1, 768, n - 300) / 16.0, np.repeat(SPECIALS.astype(np.float64), 50)]).astype(F)
    disp = disp[rng.permutation(n)]
    xy = (rng.uniform(0, 1, (n, 2)) * [1241, 376]).astype(F)
    xy[::2] = np.floor(xy[::2])
    return _ro(xy, disp)


@functools.lru_cache(maxsize=None)
def tri_specials_input():
    disp = np.tile(np.concatenate([SPECIALS, np.array([np.inf, 3.5], F)]), 9)  # 72 entries: more than a wave
    rng = np.random.default_rng(77)
    xy = (rng.uniform(0, 1, (len(disp), 2)) * [1241, 376]).astype(F)
    return _ro(xy, disp)


def _tri_equal(got, want, nan_places=False):
    """kept_xy, xyz, kept_index: lengths and bytes.  nan_places: xyz NaN at the same places, bytes elsewhere."""
    assert [len(a) for a in got] == [len(a) for a in want], ([len(a) for a in got], [len(a) for a in want])
    assert np.array_equal(_u32(got[0]), _u32(want[0]))
    assert np.array_equal(got[2], want[2])
    g, w = np.asarray(got[1]), np.asarray(want[1])
    if nan_places:
        assert np.array_equal(np.isnan(g), np.isnan(w))
        g, w = np.where(np.isnan(g), F(0), g), np.where(np.isnan(w), F(0), w)
    bad = _u32(g) != _u32(w)
    assert not bad.any(), (int(bad.sum()), g[bad.any(axis=1)][:4].tolist(), w[bad.any(axis=1)][:4].tolist())


# ================================================================================================ CPU
def _tri_args(pose, cam):
    return (POSES[pose],) + CAMERAS[cam]


def _dedup_inputs():
    """name -> (det, trk, min_d, expected kept mask or None), in file order."""
    out = {name: threshold_input(name) + (None,) for name in THRESHOLDS}
    out.update({c[0]: c[1:] for c in shape_cases()})
    out.update(special_dedup_inputs())
    return out


def _tri_inputs():
    """name -> (xy, disp, pose16, camera, expected kept mask or None, compare NaN by place), in file order."""
    out = {}
    for n, kind in mask_cases():
        xy, disp, keep = mask_input(n, kind)
        out["mask_%s_%d" % (kind, n)] = (xy, disp, POSES["rotated"], KITTI, keep, False)
    for pose in POSES:
        for cam in CAMERAS:
            out["val_%s_%s" % (pose, cam)] = value_input(pose, cam) + (POSES[pose], CAMERAS[cam], None, False)
    out["tri_specials"] = tri_specials_input() + (POSES["rotated"], KITTI, None, True)
    return out


@functools.lru_cache(maxsize=None)
def _dedup_expected(name):
    det, trk, min_d, _ = _dedup_inputs()[name]
    return _ro(GR.dedup(det, trk, min_d))


@functools.lru_cache(maxsize=None)
def _tri_expected(name):
    xy, disp, pose, cam, _, _ = _tri_inputs()[name]
    return _ro(*GR.triangulate(xy, disp, pose, *cam))


# The restatement's counters of the threshold inputs (generated once on the CPU by this file; test_threshold_inputs asserts them).
# flip_<variant>: pairs of the whole n_det x n_trk plane the variant decides differently.  to_dropped / to_kept: detected pixels the
# variant drops although the declared arithmetic keeps them / the reverse.  Only "fma" moves pairs both ways: "le" can only drop
# more by definition, "squared" (10.1f * 10.1f rounds up) likewise, and a pair that f64 keeps but the f32 statements drop needs the
# f32 distance to come out a whole ulp short: 3 of 4,000,000 candidates at 10.1, none at the other radii.
THRESHOLD_COUNTERS = {
    'thr_30': {'n': 280, 'kept': 170, 'dropped': 110, 'dropped_by_one': 110, 'at_threshold': 150, 'ulp_below': 90, 'flip_fma': 60, 'flip_f64': 77, 'flip_le': 150, 'flip_squared': 0},
    'thr_10.1': {'n': 311, 'kept': 200, 'dropped': 111, 'dropped_by_one': 111, 'at_threshold': 180, 'ulp_below': 91, 'flip_fma': 60, 'flip_f64': 116, 'flip_le': 180, 'flip_squared': 81},
    'thr_7': {'n': 280, 'kept': 170, 'dropped': 110, 'dropped_by_one': 110, 'at_threshold': 150, 'ulp_below': 90, 'flip_fma': 60, 'flip_f64': 79, 'flip_le': 150, 'flip_squared': 0},
    'thr_1': {'n': 280, 'kept': 170, 'dropped': 110, 'dropped_by_one': 110, 'at_threshold': 150, 'ulp_below': 90, 'flip_fma': 60, 'flip_f64': 60, 'flip_le': 150, 'flip_squared': 0},
}
THRESHOLD_SPREAD = {
    'thr_30': {'fma': (30, 30), 'f64': (77, 0), 'le': (150, 0), 'squared': (0, 0)},
    'thr_10.1': {'fma': (30, 30), 'f64': (115, 1), 'le': (180, 0), 'squared': (81, 0)},
    'thr_7': {'fma': (30, 30), 'f64': (79, 0), 'le': (150, 0), 'squared': (0, 0)},
    'thr_1': {'fma': (30, 30), 'f64': (60, 0), 'le': (150, 0), 'squared': (0, 0)},
}


@pytest.mark.parametrize("name", list(THRESHOLDS))
def test_threshold_inputs(name):
    det, trk, min_d = threshold_input(name)
    assert len(det) * len(trk) <= 1025 * 129
    kept, c = GR.dedup(det, trk, min_d, counters=True)
    x, y, tx, ty = det[:, 0:1], det[:, 1:2], trk[None, :, 0], trk[None, :, 1]
    dist, hit = GR._hit_plane(x, y, tx, ty, min_d)
    # decided by the pair alone: no detected pixel has a second tracked point within 1.25 min_d
    assert ((dist < F(1.25 * min_d)).sum(axis=1) == 1).all() and ((dist < F(1.25 * min_d)).sum(axis=0) == 1).all()
    spread = {}
    for v in GR.DEDUP_VARIANTS:
        h = GR._hit_plane(x, y, tx, ty, min_d, v)[1].any(axis=1)
        spread[v] = (int((h & ~hit.any(axis=1)).sum()), int((~h & hit.any(axis=1)).sum()))
    print(name, len(det), c, spread)
    assert dict(n=len(det), **c) == THRESHOLD_COUNTERS[name] and spread == THRESHOLD_SPREAD[name]
    assert c["flip_fma"] >= 50 and c["flip_f64"] >= 50 and c["at_threshold"] >= 50 and c["ulp_below"] >= 50
    assert min(spread["fma"]) >= 20
    assert c["flip_le"] == c["at_threshold"] and c["dropped_by_one"] == c["dropped"]
    if name == "thr_10.1":
        assert c["flip_squared"] >= 50
    # the oracle (a loop with an early exit) gives the same list
    assert np.array_equal(_u32(O.dedup(det, trk, min_d)), _u32(kept))


def test_dedup_shape_and_special_inputs():
    """The expected keep mask of every designed case is known from its construction; the restatement and the oracle both give it."""
    cases = shape_cases() + [(k,) + v for k, v in special_dedup_inputs().items()]
    assert {nd for nd, _ in shape_pairs()} == set(N_DET) and {nt for _, nt in shape_pairs()} == set(N_TRK)
    for nt in N_TRK:
        assert sum(1 for _, t in shape_pairs() if t == nt) >= 3
    seen = {p: 0 for p in PATTERNS}
    for name, det, trk, min_d, keep in cases:
        kept, c = GR.dedup(det, trk, min_d, counters=True)
        assert np.array_equal(_u32(kept), _u32(det[keep])), name
        assert np.array_equal(_u32(O.dedup(det, trk, min_d)), _u32(kept)), name
        assert c["dropped_by_one"] == c["dropped"] == int((~keep).sum()), name
        assert all(c["flip_" + v] == 0 for v in GR.DEDUP_VARIANTS) or name.startswith("dd_"), (name, c)
        if name.split("_")[0] + "_" + name.split("_")[1] in seen:
            seen[name.split("_")[0] + "_" + name.split("_")[1]] += 1
        elif name.split("_")[0] in seen:
            seen[name.split("_")[0]] += 1
    print(len(cases), seen)
    # 33 shapes, 5 of them with n_trk = 0 (only "none" exists there), 16 with n_trk >= 65
    assert seen == {"trk_last": 28, "trk_first": 28, "trk_64": 16, "det_last": 28, "det_first": 28, "all": 28, "none": 33}
    with np.errstate(over="ignore"):
        d = special_dedup_inputs()["dd_huge"]
        assert np.isposinf((d[0][0, 0] - d[1][0, 0]) ** 2)


TRI_COUNTERS = {
    'val_identity_kitti': {'kept': 1300, 'dropped': 200, 'dropped_minus_one': 50, 'dropped_plus_zero': 50, 'dropped_minus_zero': 50, 'dropped_nan': 50, 'kept_subnormal': 50, 'kept_inf': 0},
    'val_identity_small': {'kept': 1300, 'dropped': 200, 'dropped_minus_one': 50, 'dropped_plus_zero': 50, 'dropped_minus_zero': 50, 'dropped_nan': 50, 'kept_subnormal': 50, 'kept_inf': 0},
    'val_rotated_kitti': {'kept': 1300, 'dropped': 200, 'dropped_minus_one': 50, 'dropped_plus_zero': 50, 'dropped_minus_zero': 50, 'dropped_nan': 50, 'kept_subnormal': 50, 'kept_inf': 0},
    'val_rotated_small': {'kept': 1300, 'dropped': 200, 'dropped_minus_one': 50, 'dropped_plus_zero': 50, 'dropped_minus_zero': 50, 'dropped_nan': 50, 'kept_subnormal': 50, 'kept_inf': 0},
    'val_far_kitti': {'kept': 1300, 'dropped': 200, 'dropped_minus_one': 50, 'dropped_plus_zero': 50, 'dropped_minus_zero': 50, 'dropped_nan': 50, 'kept_subnormal': 50, 'kept_inf': 0},
    'val_far_small': {'kept': 1300, 'dropped': 200, 'dropped_minus_one': 50, 'dropped_plus_zero': 50, 'dropped_minus_zero': 50, 'dropped_nan': 50, 'kept_subnormal': 50, 'kept_inf': 0},
    'tri_specials': {'kept': 36, 'dropped': 36, 'dropped_minus_one': 9, 'dropped_plus_zero': 9, 'dropped_minus_zero': 9, 'dropped_nan': 9, 'kept_subnormal': 9, 'kept_inf': 9},
}


def test_triangulation_inputs():
    assert {n for n, k in mask_cases() if k == "all"} == set(TRI_N) == {n for n, k in mask_cases() if k == "none"}
    for k in MASKS:
        assert sum(1 for n, kk in mask_cases() if kk == k) >= 4
    for name, (xy, disp, pose, cam, keep, nan_places) in _tri_inputs().items():
        assert len(xy) <= 3073
        kxy, xyz, idx, c = GR.triangulate(xy, disp, pose, *cam, counters=True)
        if keep is not None:  # mask cases: the kept list is known from the construction
            assert np.array_equal(idx, np.flatnonzero(keep)) and c["kept"] == int(keep.sum()), name
        _tri_equal(O.triangulate(xy, disp, pose, *cam), (kxy, xyz, idx), nan_places)
        assert nan_places or not np.isnan(xyz).any(), name
        if name in TRI_COUNTERS or keep is None:
            print(name, c)
            assert c == TRI_COUNTERS[name], name
    # chunk-boundary properties of the masks that the compaction has to carry `base` across
    assert keep_mask(2049, "one_per_chunk_last_lane").nonzero()[0].tolist() == [1023, 2047, 2048]
    assert not keep_mask(2049, "chunk0_empty")[:1024].any() and keep_mask(2049, "chunk0_empty")[1024:2048].all()


@pytest.mark.parametrize("pose", list(POSES))
def test_value_inputs_decide_the_arithmetic(pose):
    """At least 1,000 kept points per pose, and the restatement's acc32, q_first and recip each change more than 25 % of them.  The one
    exception is exact: under the identity pose I (Q v) and (I Q) v are the same four numbers, so q_first changes nothing there; the
    product order is decided by the two other poses."""
    for cam in CAMERAS:
        xy, disp = value_input(pose, cam)
        base = GR.triangulate(xy, disp, POSES[pose], *CAMERAS[cam])
        assert len(base[2]) >= 1000
        for v in ("acc32", "q_first", "recip"):
            alt = GR.triangulate(xy, disp, POSES[pose], *CAMERAS[cam], variant=v)
            changed = (_u32(alt[1]) != _u32(base[1])).any(axis=1).mean()
            print(pose, cam, v, "changes %.1f %% of %d kept points" % (100 * changed, len(base[2])))
            if pose == "identity" and v == "q_first":
                assert changed == 0
            else:
                assert changed > 0.25, (pose, cam, v, changed)


def test_inputs_tell_the_variants_apart():
    """Every misreading changes the bytes the restatement returns for the inputs named here; "div64" changes none."""
    for v, names in (("fma", list(THRESHOLDS)), ("f64", list(THRESHOLDS)), ("le", list(THRESHOLDS)), ("squared", ["thr_10.1"])):
        for name in names:
            det, trk, min_d = threshold_input(name)
            assert not np.array_equal(GR.dedup(det, trk, min_d, variant=v), _dedup_expected(name)), (v, name)
    values = ["val_%s_%s" % (p, c) for p in POSES for c in CAMERAS]
    for v, names in (("acc32", values), ("q_first", [n for n in values if "identity" not in n]), ("recip", values),
                     ("ge0", values + ["tri_specials", "mask_none_64", "mask_alternate_lanes_1025"])):
        for name in names:
            xy, disp, pose, cam, _, _ = _tri_inputs()[name]
            alt = GR.triangulate(xy, disp, pose, *cam, variant=v)
            base = _tri_expected(name)
            assert len(alt[2]) != len(base[2]) or not np.array_equal(_u32(alt[1]), _u32(base[1])), (v, name)
    # "ge0" is decided by the +0.0 and -0.0 entries: exactly those join the kept list
    xy, disp = value_input("rotated", "kitti")
    extra = np.setdiff1d(GR.triangulate(xy, disp, POSES["rotated"], *KITTI, variant="ge0")[2], _tri_expected("val_rotated_kitti")[2])
    assert len(extra) == 100 and (disp[extra] == 0).all() and np.signbit(disp[extra]).sum() == 50
    # "div64": the quotient of two f32 in f64 (53 bits >= 2 * 24 + 2) rounded to f32 IS the correctly rounded f32 quotient, so no
    # input can tell the two apart
    for name, (xy, disp, pose, cam, _, nan_places) in _tri_inputs().items():
        _tri_equal(GR.triangulate(xy, disp, pose, *cam, variant="div64"), _tri_expected(name), nan_places)


def _ulp(v):
    v = F(abs(v))
    return float(np.nextafter(v, F(np.inf))) - float(v)


def test_restatement_rows_against_exact_rational_sums():
    """64 points x 3 poses: the four row values of the restatement against the exact rational sum of the f32 inputs, rounded to f32
    (within 1 ulp: the f64 accumulation rounds three times before the f32 rounding); and the 16 known answers of the golden fixture
    as test_constants.py checks them."""
    rng = np.random.default_rng(9)
    xy = (rng.uniform(0, 1, (64, 2)) * [1241, 376]).astype(F)
    d = (rng.integers(1, 768, 64) / 16.0).astype(F)
    for pose in POSES.values():
        M = GR.reprojection_matrix(pose, *KITTI)
        rows = GR._rows(M, xy[:, 0], xy[:, 1], d)
        for i in range(64):
            for r in range(4):
                exact = (Fraction(float(M[r, 0])) * Fraction(float(xy[i, 0])) + Fraction(float(M[r, 1])) * Fraction(float(xy[i, 1]))
                         + Fraction(float(M[r, 2])) * Fraction(float(d[i])) + Fraction(float(M[r, 3])))
                want = F(float(exact))
                assert abs(float(rows[r, i]) - float(want)) <= _ulp(want), (i, r, rows[r, i], want)
        # M itself: each element against the exact rational sum
        Q = GR.reprojection_q(*KITTI)
        for i in range(4):
            for j in range(4):
                exact = sum(Fraction(float(pose[i, k])) * Fraction(float(Q[k, j])) for k in range(4))
                assert abs(float(M[i, j]) - float(F(float(exact)))) <= _ulp(F(float(exact)))
    import json
    import os
    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "constants_golden.json")))
    assert len(gold["triangulation"]) == 16
    for q in gold["q"]:
        Q = GR.reprojection_q(q["focal"], q["cx"], q["cy"], q["baseline"])
        assert np.allclose(Q.ravel(), q["Q"], rtol=1e-6)
    for c in gold["triangulation"]:
        q = gold["q"][c["camera"]]
        kxy, xyz, kidx = GR.triangulate([[c["x"], c["y"]]], [c["disp"]], c["pose16"], q["focal"], q["cx"], q["cy"], q["baseline"])
        assert len(kidx) == 1 and np.allclose(xyz[0], c["xyz"], rtol=2e-6, atol=1e-5), (xyz, c["xyz"])


def _rodrigues(rv):
    th = np.linalg.norm(rv)
    k = rv / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return (np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K).astype(F)


def test_chain_matrix_under_hmat_from_R_t():
    """No oracle_lib entry exposes the keyframe's matrix or its points, so the chain is compared through the points: O.triangulate and
    the restatement, both under hmat_from_R_t(R, t), for 5 rotations (and hmat against the exact rational -R^T t).  The device side of
    host/chain_math.h stays covered by the stream keys only."""
    rng = np.random.default_rng(21)
    xy, disp = value_input("rotated", "kitti")
    for k in range(5):
        R = _rodrigues(rng.normal(size=3) * (0.02 + 0.3 * k))
        t = (rng.normal(size=3) * [0.5, 0.2, 3.0 + 40 * k]).astype(F)
        h = GR.hmat_from_R_t(R, t)
        assert np.array_equal(h[:3, :3], R.T) and h[3].tolist() == [0, 0, 0, 1]
        for i in range(3):
            exact = sum(Fraction(float(-R[kk, i])) * Fraction(float(t[kk])) for kk in range(3))
            assert abs(float(h[i, 3]) - float(F(float(exact)))) <= _ulp(F(float(exact)))
        _tri_equal(O.triangulate(xy, disp, h, *KITTI), GR.triangulate(xy, disp, h, *KITTI))


# ================================================================================================ GPU: the stand-alone entries
def _dedup_pass(ctx, names):
    inputs = _dedup_inputs()
    for name in names:
        det, trk, min_d, keep = inputs[name]
        got = ctx.dedup(det, trk, min_d)
        want = _dedup_expected(name)
        if keep is not None:
            assert np.array_equal(_u32(want), _u32(det[keep])), name
        assert got.shape == want.shape, (name, got.shape, want.shape)
        assert np.array_equal(_u32(got), _u32(want)), name


@gpu
def test_hip_dedup_every_input_forward_then_reverse(ctx):
    """svo_dedup on every dedup input in file order, then once more in reverse order on the same context: the arrival counter behind
    svo_arrive_next is cumulative, so a launch's target depends on everything launched before it."""
    names = list(_dedup_inputs())
    assert len(names) == 4 + 189 + 3
    _dedup_pass(ctx, names)
    _dedup_pass(ctx, names[::-1])


def _tri_pass(ctx, names):
    inputs = _tri_inputs()
    for name in names:
        xy, disp, pose, cam, keep, nan_places = inputs[name]
        try:
            _tri_equal(ctx.triangulate(xy, disp, pose, *cam), _tri_expected(name), nan_places)
        except AssertionError as e:
            raise AssertionError(name + ": " + str(e)) from None


@gpu
def test_hip_triangulate_every_input_forward_then_reverse(ctx):
    names = list(_tri_inputs())
    assert len(names) == 22 + 7 * 8 + 6 + 1
    _tri_pass(ctx, names)
    _tri_pass(ctx, names[::-1])


CANARY = 0x7F81BEEF  # a signalling NaN pattern no computation here produces


def _raw_triangulate(ctx, xy, disp, pose, cam, with_index):
    n = len(xy)
    kxy = np.full((n, 2), CANARY, np.uint32).view(F)
    xyz = np.full((n, 3), CANARY, np.uint32).view(F)
    kidx = np.full(n, -77, np.int32)
    m = C.c_int(-5)
    pose = np.ascontiguousarray(pose, F)
    rc = ctx.L.svo_triangulate(ctx.h, xy.ctypes.data_as(C.c_void_p), disp.ctypes.data_as(C.c_void_p), n, pose.ctypes.data_as(C.c_void_p),
                               C.c_float(cam[0]), C.c_float(cam[1]), C.c_float(cam[2]), C.c_float(cam[3]),
                               kxy.ctypes.data_as(C.c_void_p), xyz.ctypes.data_as(C.c_void_p),
                               kidx.ctypes.data_as(C.c_void_p) if with_index else None, C.byref(m))
    assert rc == 0, (rc, ctx.L.svo_last_error(ctx.h))
    return kxy, xyz, kidx, m.value


@gpu
@pytest.mark.parametrize("name", ["val_rotated_kitti", "mask_alternate_waves_2049", "mask_none_1025", "mask_last_3073"])
def test_hip_triangulate_without_kept_index(ctx, name):
    """kept_index = NULL gives the same kept_xy and xyz; with every host buffer pre-filled by a canary, the entries at and beyond n_kept
    are unchanged (and kept_index is not written at all)."""
    xy, disp, pose, cam, _, _ = _tri_inputs()[name]
    want = _tri_expected(name)
    for with_index in (True, False):
        kxy, xyz, kidx, m = _raw_triangulate(ctx, xy, disp, pose, cam, with_index)
        assert m == len(want[2])
        assert np.array_equal(_u32(kxy[:m]), _u32(want[0])) and np.array_equal(_u32(xyz[:m]), _u32(want[1]))
        assert (_u32(kxy[m:]) == CANARY).all() and (_u32(xyz[m:]) == CANARY).all()
        if with_index:
            assert np.array_equal(kidx[:m], want[2]) and (kidx[m:] == -77).all()
        else:
            assert (kidx == -77).all()


SVO_ERR_INVALID, SVO_ERR_CAPACITY = -1, -3


@gpu
def test_hip_dedup_capacity():
    """A context asked for max_batch = 1, max_candidates = 256.  svo_create raises a candidate bound below 1024 to 1024 (ctx.hip), so the
    bound the dedup flags live under is 1024, not the 256 asked for: 257 detected pixels are ANSWERED (correctly), and the refusal
    comes at 1025, with SVO_ERR_CAPACITY and the "too many detected corners" message; a 1024- and a 256-pixel call after the refusal are
    answered correctly.  No count of the triangulation inputs (up to 3073) is refused for workspace by the session context."""
    import stereo_vo_amd as S
    small = S.Context(640, 480, max_batch=1, max_candidates=256)
    try:
        cases = {nd: shape_input(nd, 65, "trk_64") for nd in (256, 257, 1024, 1025)}
        det, trk, min_d, keep = cases[257]
        assert np.array_equal(_u32(small.dedup(det, trk, min_d)), _u32(det[keep]))
        det, trk, min_d, keep = cases[1025]
        out, m = np.empty_like(det), C.c_int(-5)
        rc = small.L.svo_dedup(small.h, det.ctypes.data_as(C.c_void_p), 1025, trk.ctypes.data_as(C.c_void_p), 65, C.c_float(min_d),
                               out.ctypes.data_as(C.c_void_p), C.byref(m))
        assert rc == SVO_ERR_CAPACITY and b"too many detected corners" in small.L.svo_last_error(small.h)
        for nd in (1024, 256):
            det, trk, min_d, keep = cases[nd]
            assert np.array_equal(_u32(small.dedup(det, trk, min_d)), _u32(det[keep])), nd
    finally:
        small.close()


@gpu
def test_hip_argument_checks(ctx):
    """n < 0, a null n_kept and a null xy with n > 0 are refused with SVO_ERR_INVALID by both entries; a correct call follows each."""
    det, trk, min_d, keep = shape_input(5, 65, "trk_64")
    xy, disp, pose, cam, _, _ = _tri_inputs()["mask_alternate_lanes_65"]
    pose = np.ascontiguousarray(pose, F)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    out2, out3, m = np.empty((65, 2), F), np.empty((65, 3), F), C.c_int(0)
    L, h = ctx.L, ctx.h
    fl = [C.c_float(v) for v in cam]
    for bad in (lambda: L.svo_dedup(h, p(det), -1, p(trk), 65, C.c_float(min_d), p(out2), C.byref(m)),
                lambda: L.svo_dedup(h, p(det), 5, p(trk), -1, C.c_float(min_d), p(out2), C.byref(m)),
                lambda: L.svo_dedup(h, p(det), 5, p(trk), 65, C.c_float(min_d), p(out2), None),
                lambda: L.svo_dedup(h, None, 5, p(trk), 65, C.c_float(min_d), p(out2), C.byref(m)),
                lambda: L.svo_dedup(h, p(det), 5, None, 65, C.c_float(min_d), p(out2), C.byref(m)),
                lambda: L.svo_triangulate(h, p(xy), p(disp), -1, p(pose), *fl, p(out2), p(out3), None, C.byref(m)),
                lambda: L.svo_triangulate(h, p(xy), p(disp), 65, p(pose), *fl, p(out2), p(out3), None, None),
                lambda: L.svo_triangulate(h, None, p(disp), 65, p(pose), *fl, p(out2), p(out3), None, C.byref(m)),
                lambda: L.svo_triangulate(h, p(xy), None, 65, p(pose), *fl, p(out2), p(out3), None, C.byref(m)),
                lambda: L.svo_triangulate(h, p(xy), p(disp), 65, None, *fl, p(out2), p(out3), None, C.byref(m))):
        assert bad() == SVO_ERR_INVALID
        assert len(L.svo_last_error(h)) > 0
        assert np.array_equal(_u32(ctx.dedup(det, trk, min_d)), _u32(det[keep]))
        _tri_equal(ctx.triangulate(xy, disp, pose, *cam), _tri_expected("mask_alternate_lanes_65"))


# ================================================================================================ GPU: the fused forms the pipelines run
def _params(S, p, md, maxc, parallax=None):
    pp = S.pipeline_default_params()
    pp.cam.focal, pp.cam.cx, pp.cam.cy, pp.cam.baseline = p.focal, p.cx, p.cy, p.baseline
    pp.width, pp.height = p.width, p.height
    pp.max_corners, pp.min_feature_distance, pp.max_features, pp.window_size = maxc, md, 1000, 5
    pp.ba_max_time_s = 0.0  # deterministic: iteration cap only (SURVEY C-10)
    if parallax is not None:
        pp.parallax_thresh = parallax
    return pp


class _Lanes:
    """A Pipeline (one lane) or a PipelineGroup behind one interface: frames are handed over one at a time."""

    def __init__(self, S, ctx, pp, lanes, group):
        self.lanes, self.pp = lanes, pp
        self.g = S.PipelineGroup(ctx, pp, lanes) if group else S.Pipeline(ctx, pp)
        self.group = group

    def step(self, Ls, Rs):
        if self.group:
            res = self.g.process_batch(np.stack(Ls)[:, None], np.stack(Rs)[:, None])
            return [r[0] for r in res]
        return [self.g.process_batch(Ls[0][None], Rs[0][None])[0]]

    def tracked(self, lane):
        return self.g.get_tracked(lane) if self.group else self.g.tracked()

    def close(self):
        self.g.close()


def _check_keyframe(ctx, pp, left, right, res, ids, xy, prev_max):
    """The tracked list after a keyframe = the inliers (ids that existed before), then the new features = corner_detect -> geom_ref.dedup
    against the inliers -> kept where the dense disparity map is > 0 at (int(x), int(y)) (SURVEY C-13), in order."""
    old = ids <= prev_max
    n_in = int(old.sum())
    assert old[:n_in].all() and (np.diff(ids) > 0).all()
    assert np.array_equal(ids[n_in:], prev_max + 1 + np.arange(len(ids) - n_in))  # contiguous and increasing
    det = ctx.corner_detect(left, pp.max_corners, pp.quality, pp.min_feature_distance)
    fresh = GR.dedup(det, xy[:n_in], pp.min_feature_distance)
    disp = ctx.stereo_bm(left, right)
    want = fresh[disp[fresh[:, 1].astype(int), fresh[:, 0].astype(int)] > 0]
    assert res.n_detected == len(det) and res.n_inliers == n_in
    assert res.n_new == len(want) == len(ids) - n_in, (res.n_new, len(want), len(ids) - n_in)
    assert np.array_equal(_u32(xy[n_in:]), _u32(want))
    return n_in, len(fresh), len(want)


def _run_stream(ctx, lanes_obj, streams, n_frames):
    """streams: per lane (L, R) image stacks.  Returns per lane the list of (frame, n_inliers, n_after_dedup, n_new) of its keyframes."""
    prev_max = [-1] * lanes_obj.lanes
    out = [[] for _ in range(lanes_obj.lanes)]
    for k in range(n_frames):
        res = lanes_obj.step([s[0][k] for s in streams], [s[1][k] for s in streams])
        for l, r in enumerate(res):
            if r.is_keyframe:
                ids, xy = lanes_obj.tracked(l)
                out[l].append((k,) + _check_keyframe(ctx, lanes_obj.pp, streams[l][0][k], streams[l][1][k], r, ids, xy, prev_max[l]))
                if len(ids):
                    prev_max[l] = max(prev_max[l], int(ids.max()))
    return out


STREAM_SEEDS = (0x5EED0200, 0x5EED025D, 0x5EED027C)  # three of the seeds whose 8 frames hold 3 keyframes (oracle pipeline, CPU)


@gpu
@pytest.mark.parametrize("form", ["pipeline", "group_same_stream", "group_three_seeds"])
def test_hip_keyframe_lists_equal_composed_references(ctx, form):
    """svo_triangulate_block<256, true> behind the sparse stereo (Pipeline) and stereo_triangulate_group_kernel<64> with the dedup
    folded in as "duplicate => disparity 0" (PipelineGroup) against the composition of three separately pinned pieces.  max_features
    is 1000: nothing is truncated (n_new equals the derived length)."""
    import stereo_vo_amd as S
    from test_pipeline import _seq
    if form == "group_three_seeds":
        seqs = [_seq(8, seed=s) for s in STREAM_SEEDS]
    else:
        seqs = [_seq(8)] * (1 if form == "pipeline" else 3)
    lanes = _Lanes(S, ctx, _params(S, seqs[0][0], 12.0, 300), len(seqs), form != "pipeline")
    try:
        got = _run_stream(ctx, lanes, [(s[1], s[2]) for s in seqs], 8)
    finally:
        lanes.close()
    print(form, got)
    for l, kfs in enumerate(got):
        assert len(kfs) >= 3, (l, kfs)
        assert kfs[0][1] == 0 and all(n_in > 0 and fresh < 300 for _, n_in, fresh, _ in kfs[1:])  # later keyframes do dedup something
    if form == "group_same_stream":
        assert got[0] == got[1] == got[2]


def static_pair(seed=0):
    """A textured block on a flat background, the right image the left shifted by 13 px: every corner of the left image has a valid
    disparity (asserted on the CPU with the StereoBM restatement)."""
    h, w = 160, 496
    rng = np.random.default_rng(seed)
    tex = np.kron(rng.integers(0, 255, (h // 4 + 1, w // 4 + 30)), np.ones((4, 4))).astype(np.uint8)
    big = np.full((h, w + 40), 128, np.uint8)
    big[24:h - 24, 100:w - 20] = tex[24:h - 24, 100:w - 20]
    return np.ascontiguousarray(big[:, 20:20 + w]), np.ascontiguousarray(big[:, 33:33 + w])


def test_empty_tail_pairs_on_the_cpu():
    """(a) The mirrored left image as the right image still leaves 7 of 242 corners with a disparity, a flat right image leaves none
    (restatement and oracle).  (b) One parameter feeds the detector's spacing and the dedup, so with min_feature_distance >= the image
    diagonal a frame has one corner and is skipped (fewer than 4, :23-25); and on the moving streams no keyframe has all corners within
    the distance of an inlier (5 seeds x 9 distances from 70 to 150 searched).  The all-duplicates keyframe is therefore built from a
    static pair whose corners all have a disparity, with parallax_thresh = -1 so that the second, identical frame is a keyframe: every
    corner is then at distance 0 from the inlier it became."""
    import stereo_bm_ref as SR
    from test_pipeline import _seq, _ora_pipe
    p, L, R = _seq(2)
    c = O.corner_detect(L[0], 300, 0.1, 12.0)
    at = lambda d: d[c[:, 1].astype(int), c[:, 0].astype(int)]
    assert len(c) == 242 and int((at(SR.stereo_bm(L[0], np.ascontiguousarray(L[0][:, ::-1]), 48, 21)) > 0).sum()) == 7
    flat = np.full_like(L[0], 90)
    assert not (at(SR.stereo_bm(L[0], flat, 48, 21)) > 0).any() and not (at(O.stereo_bm(L[0], flat)) > 0).any()
    assert len(O.corner_detect(L[0], 300, 0.1, float(np.hypot(496, 160)))) == 1
    Ls, Rs = static_pair()
    c = O.corner_detect(Ls, 300, 0.1, 12.0)
    assert len(c) == 191 and (SR.stereo_bm(Ls, Rs, 48, 21)[c[:, 1].astype(int), c[:, 0].astype(int)] > 0).all()
    o = _ora_pipe(p, min_feature_distance=12.0, max_features=1000, parallax_thresh=-1.0)
    res = [o.process(Ls, Rs) for _ in range(3)]
    assert [(r.n_detected, r.n_tracked, r.n_inliers, r.n_new, r.is_keyframe) for r in res] == [(191, 0, 0, 191, 1)] + [(191, 191, 191, 0, 1)] * 2
    o = _ora_pipe(p, min_feature_distance=12.0, max_features=1000)
    res = [o.process(L[0], flat), o.process(L[1], R[1])]
    assert [(r.n_detected, r.n_tracked, r.n_inliers, r.n_new, r.is_keyframe) for r in res] == [(242, 0, 0, 0, 1), (257, 0, 0, 164, 1)]


@gpu
@pytest.mark.parametrize("group", [False, True], ids=["pipeline", "group"])
def test_hip_keyframe_without_any_disparity(ctx, group):
    """(a) A first frame whose right image is flat: no corner has a disparity, the tail runs with nothing kept.  The keyframe has
    n_new == 0 and an empty tracked list; the next frame tracks nothing, is a keyframe again (nothing tracked = everything lost) and
    gives the composed reference's list."""
    import stereo_vo_amd as S
    from test_pipeline import _seq
    p, L, R = _seq(3)
    R = R.copy()
    R[0] = 90
    n = 3 if group else 1
    lanes = _Lanes(S, ctx, _params(S, p, 12.0, 300), n, group)
    try:
        got = _run_stream(ctx, lanes, [(L, R)] * n, 3)
    finally:
        lanes.close()
    for kfs in got:
        assert kfs[:2] == [(0, 0, 242, 0), (1, 0, 257, 164)], kfs


@gpu
@pytest.mark.parametrize("group", [False, True], ids=["pipeline", "group"])
def test_hip_keyframe_with_only_duplicates(ctx, group):
    """(b) A static pair, parallax_thresh = -1: the second and third frames are keyframes whose 191 corners are all duplicates of the
    191 inliers: n_new == 0 and the tracked list is the inliers.  In the group this is "duplicate => disparity 0" in every workgroup."""
    import stereo_vo_amd as S
    from test_pipeline import _seq
    p, _, _ = _seq(1)
    Ls, Rs = static_pair()
    n = 3 if group else 1
    lanes = _Lanes(S, ctx, _params(S, p, 12.0, 300, parallax=-1.0), n, group)
    stream = (np.stack([Ls] * 3), np.stack([Rs] * 3))
    try:
        got = _run_stream(ctx, lanes, [stream] * n, 3)
        ids, xy = lanes.tracked(0)
    finally:
        lanes.close()
    for kfs in got:
        assert kfs == [(0, 0, 191, 191), (1, 191, 0, 0), (2, 191, 0, 0)], kfs
    assert np.array_equal(ids, np.arange(191))
