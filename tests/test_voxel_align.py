"""The voxel map align (include/svo.h, "Voxel map align") against the restatement tests/voxel_align_ref.py, with ==.

CPU: the restatement's two routes agree on every scene; each deliberate misreading of the contract changes the sums of a stated
scene; the constructed scenes are what they were built to be; the pure entries and the refusals that need no context; the loop on
the restatement alone; host/voxel_align.h under ASan + UBSan (tests/sanitize/voxel_align_args_test.cpp).
GPU: all 32 words into a sentinel-filled guarded buffer equal the restatement run on the DOWNLOADED table, the table's bytes and the
map's counters are unchanged after every call; svo_voxel_map_align equals the restatement's loop in every bit.

Main scene (tests/test_voxel_map.py: 160 x 80, 12,800 records per cloud): the map holds cloud A under TRUTH, a pose7 whose
camera->world transform is rot_y(0.7), shift (1.5, 0, -2).  Cloud B (the second view: the same geometry measured again, with other
disparity noise and intensities) has TRUTH as its true pose and is aligned from START(vs): TRUTH's camera->world transform shifted by
0.5 voxel * (0.6, -0.5, 0.62) and turned by 0.01 rad * (0.5, 0.7, -0.5).  On the restatement (translation error in map units, rotation
error in radians, before -> after 10 iterations, status MAX_ITERS each; cost word first -> last):
  0.05 m  0.02493 -> 0.02079   0.00995 -> 0.00441   6196599436 -> 4957683221
  0.1 m   0.04986 -> 0.03809   0.00995 -> 0.00660   14503015569 -> 10886768750
  0.25 m  0.12465 -> 0.07625   0.00995 -> 0.00909   51601922114 -> 32266348082
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import voxel_align_ref as A
import voxel_ref as V
import test_voxel_map as T
from test_host_sanitizers import _run_sanitized

SIZES = ((0.05, 14), (0.1, 14), (0.25, 12))  # voxel size, table log2 (one cloud)
TRUTH = A.to_pose7([math.cos(0.35), 0.0, math.sin(0.35), 0.0], [1.5, 0.0, -2.0])
SENT = 0x5A5A5A5A5A5A5A5A
VS, LOG2 = 0.25, 8  # the constructed scenes: q = x * 4 exactly
F32 = np.float32


def START(vs):
    return A.displaced(TRUTH, [0.5 * vs * c for c in (0.6, -0.5, 0.62)], [0.01 * c for c in (0.5, 0.7, -0.5)])


def _m(pose7):
    """A pose7's camera->world matrix by the library's own pure conversion (its bits are the contract's)."""
    from stereo_vo_amd import api
    return api.pose7_to_cam_to_world(np.asarray(pose7, np.float64)).reshape(12)


def ident(t=(0.0, 0.0, 0.0)):
    m = T.IDENT.copy()
    m[3], m[7], m[11] = t
    return m


# ----------------------------------------------------------------------------------------------------- tables without a GPU
def cpu_table(steps, vs, md, lg):
    """The download of a 2^lg table after the steps ("insert" | "remove", records, m12): each step's voxels in ascending key order,
    each placed by the insert's linear probing; a removal is the exact inverse of an earlier insert of the same records."""
    cap = 1 << lg
    d = {"keys": np.full(cap, V.EMPTY, np.uint64)}
    for n in ("ci", "sx", "sy", "sz"):
        d[n] = np.zeros(cap, np.uint64)
    for kind, pts, m in steps:
        t = V.insert_np(pts, m, vs, md)
        for i, k in enumerate(t.keys.tolist()):
            h = V.fmix64(k) & (cap - 1)
            for _ in range(V.MAX_PROBES):
                if int(d["keys"][h]) in (V.EMPTY, k):
                    break
                h = (h + 1) & (cap - 1)
            else:
                assert kind == "insert"
                continue  # dropped
            if kind == "insert":
                d["keys"][h] = k
                for n in ("ci", "sx", "sy", "sz"):
                    d[n][h] += getattr(t, n)[i]
            else:
                assert int(d["keys"][h]) == k and all(int(d[n][h]) >= int(getattr(t, n)[i]) for n in ("ci", "sx", "sy", "sz"))
                for n in ("ci", "sx", "sy", "sz"):
                    d[n][h] -= getattr(t, n)[i]
    return d


def rec(cell, frac=(0.5, 0.5, 0.5), tag=0x40000000):
    """One record inside voxel `cell` at VS, at the dyadic fraction `frac` of it: exact in f32."""
    xyz = [F32((c + f) * VS) for c, f in zip(cell, frac)]
    assert all(float(v) == (c + f) * VS for v, c, f in zip(xyz, cell, frac))
    return V.records([xyz[0]], [xyz[1]], [xyz[2]], np.array([tag], np.uint32))


def cat(*parts):
    return np.concatenate(parts)


@functools.lru_cache(maxsize=None)
def wrap_cells():
    """Four voxels (z = 8) whose keys have the home slots 254, 255, 255, 254 of a 2^8 table, in this order: inserted one after the
    other they take the slots 254, 255, 0 and 1, so the last one sits behind a run that wraps past the end of the table."""
    want, out, used = [254, 255, 255, 254], [], set()
    for home in want:
        for i in range(-400, 400):
            for j in range(-3, 4):
                c = (i, j, 8)
                if c not in used and V.fmix64(A.key_of(c)) & 255 == home and not any(max(abs(a - b) for a, b in zip(c, u)) <= 2 for u in used):
                    out.append(c)
                    used.add(c)
                    break
            else:
                continue
            break
    assert len(out) == 4
    return out


@functools.lru_cache(maxsize=None)
def small_scenes():
    """name -> (steps, records, m12, max_depth, params, expectation(words, matched keys)) at VS in a 2^8 table."""
    P = lambda **kw: A.default_params(VS, min_matches=6, **kw)
    K = A.key_of
    E = V.EMPTY
    out = {}
    near, nxt = (3, 2, 8), (4, 2, 8)
    # a point on a voxel face belongs to the upper voxel; its nearest mean is across the face
    face = [("insert", cat(rec(near), rec((2, 2, 8), (0.75, 0.5, 0.5))), ident())]
    out["face_reach1"] = (face, rec(near, (0.0, 0.5, 0.5)), ident(), 0.0, P(), lambda w, k: w[17] == 1 and k[0] == K((2, 2, 8)))
    out["face_reach0"] = (face, rec(near, (0.0, 0.5, 0.5)), ident(), 0.0, P(reach=0), lambda w, k: w[17] == 1 and k[0] == K(near))
    # two neighbours at bit-equal d2: the smallest key wins, in either table order
    for name, order in (("tie_ab", ((2, 2, 8), near)), ("tie_ba", (near, (2, 2, 8)))):
        steps = [("insert", rec(c), ident()) for c in order]
        out[name] = (steps, rec(near, (0.0, 0.5, 0.5)), ident(), 0.0, P(), lambda w, k: w[17] == 1 and k[0] == K((2, 2, 8)))
    # the nearest candidate below min_count, a farther one qualifying
    steps = [("insert", cat(rec(near), rec(nxt, (0.25, 0.5, 0.5)), rec(nxt, (0.75, 0.5, 0.5))), ident())]
    out["below_min_count"] = (steps, rec(near, (0.5, 0.5, 0.75)), ident(), 0.0, P(min_count=2), lambda w, k: w[17] == 1 and k[0] == K(nxt))
    # a carved nearest candidate (a removal's emptied voxel is exactly a carved one: the key stays, the count is 0)
    steps = [("insert", cat(rec(near), rec(nxt)), ident()), ("remove", rec(near), ident())]
    out["carved_nearest"] = (steps, rec(near, (0.5, 0.5, 0.75)), ident(), 0.0, P(), lambda w, k: w[17] == 1 and k[0] == K(nxt))
    # a candidate whose key sits after a run that wraps past the end of the table
    wc = wrap_cells()
    steps = [("insert", rec(c), ident()) for c in wc]
    out["wrapped_run"] = (steps, rec(wc[3], (0.5, 0.75, 0.5)), ident(), 0.0, P(reach=0), lambda w, k: w[17] == 1 and k[0] == K(wc[3]))
    # d2 == D2 matches; the double above it is far (the matrix shifts y by 2^-28, so d2 = 2^-4 + 2^-56)
    one = [("insert", rec(near), ident())]
    out["d2_equals_D2"] = (one, rec(nxt), ident(), 0.0, P(max_dist=0.25), lambda w, k: w[17:21] == [1, 0, 0, 0] and w[16] == 1 << 24)
    out["d2_above_D2"] = (one, rec(nxt), ident((0.0, 2.0 ** -28, 0.0)), 0.0, P(max_dist=0.25), lambda w, k: w[17:21] == [0, 0, 0, 1])
    # q_r at both ends of rule 1's range (x = 0.5, shifted by the matrix)
    lo, hi = -262144.25, 262143.25
    for name, t0, kept in (("q_low_end", lo, True), ("q_below_low_end", np.nextafter(lo, -np.inf), False),
                           ("q_high_end", hi, False), ("q_below_high_end", np.nextafter(hi, 0.0), True)):
        out[name] = (one, rec((2, 2, 8), (0.0, 0.5, 0.5)), ident((float(t0), 0.0, 0.0)), 0.0, P(),
                     (lambda w, k: w[17:21] == [0, 0, 1, 0]) if kept else (lambda w, k: w[17:21] == [0, 1, 0, 0]))
    # |x| = 1024 and the float below it; a NaN z
    f = lambda x, y, z: V.records([F32(x)], [F32(y)], [F32(z)], np.array([0], np.uint32))
    below = np.nextafter(F32(1024), F32(0))
    for name, p, kept in (("x_1024", f(1024, 1, 2), False), ("x_minus_1024", f(-1024, 1, 2), False), ("x_below_1024", f(below, 1, 2), True),
                          ("y_1024", f(1, 1024, 2), False), ("y_below_1024", f(1, -below, 2), True), ("z_1024", f(1, 1, 1024), False),
                          ("z_below_1024", f(1, 1, below), True), ("z_nan", f(1, 1, np.nan), False), ("x_nan", f(np.nan, 1, 2), False)):
        out[name] = (one, p, ident(), 0.0, P(), (lambda w, k: w[17:21] == [0, 0, 1, 0]) if kept else (lambda w, k: w[17:21] == [0, 1, 0, 0]))
    # a term at Q_S's half, both signs: x * 2^16 = +-32768.5
    h = 0.5 + 2.0 ** -17
    for name, x, cell, want in (("half_plus", h, (2, 2, 8), 32769), ("half_minus", -h, (-3, 2, 8), -32768)):
        out[name] = ([("insert", rec(cell), ident())], f(x, 0.625, 2.125), ident(), 0.0, P(), lambda w, k, want=want: w[17] == 1 and w[1] == want)
    # a cloud that matches nothing, and one rejected entirely
    out["nothing_matches"] = (one, cat(*[rec((20 + 3 * i, 2, 8)) for i in range(70)]), ident(), 0.0, P(), lambda w, k: w[17:21] == [0, 0, 70, 0])
    out["all_rejected"] = (one, T._reject(130), ident(), 0.0, P(), lambda w, k: w[17:21] == [0, 130, 0, 0] and not any(w[:17]))
    out["max_depth"] = (one, cat(rec(near), rec((3, 2, 9))), ident(), 2.2, P(), lambda w, k: w[17:21] == [1, 1, 0, 0])
    return out


@functools.lru_cache(maxsize=None)
def full_table():
    """3,000 distinct voxels at 0.1 m into 2^8 slots (tests/test_voxel_remove.py): every slot is taken."""
    p = T._voxel_records([(i % 10, (i // 10) % 10 - 5, 10 + i // 100) for i in range(3000)])
    absent = T._voxel_records([(50 + i, 0, 60) for i in range(130)])
    return p, absent


@functools.lru_cache(maxsize=None)
def main_table(vs, lg, reverse=False):
    A_ = T.main_scene()
    return cpu_table([("insert", A_[::-1] if reverse else A_, _m(TRUTH))], vs, 0.0, lg)


@functools.lru_cache(maxsize=None)
def tail_clouds():
    """name -> n records for the wavefront and workgroup tails: records of cloud B that match at 0.1 m under TRUTH, with all, the
    first, the last or none of them left where they are (the others moved 500 m away: unmatched)."""
    B = T.second_cloud()
    prm = A.default_params(0.1)
    _, keys = A.sums_np(main_table(0.1, 14), B, _m(TRUTH), 0.1, 0.0, prm, detail=True)
    good = B[keys != np.uint64(V.EMPTY)]
    out = {}
    for n in (1, 63, 64, 65, 256, 257):
        for which in ("all", "first", "last", "none"):
            p = good[1000:1000 + n].copy()
            away = np.ones(n, bool)
            if which == "all":
                away[:] = False
            elif which == "first":
                away[0] = False
            elif which == "last":
                away[-1] = False
            p["x"][away] += F32(500)
            out[f"{which}_{n}"] = (p, {"all": n, "first": 1, "last": 1, "none": 0}[which])
    return out


# ===================================================================================================== CPU
def test_the_two_routes_of_the_restatement_agree_on_every_scene():
    B = T.second_cloud()
    for vs, lg in SIZES:
        for reach in (0, 1):
            for mc in (1, 3):
                prm = A.default_params(vs, reach=reach, min_count=mc)
                w = A.both(main_table(vs, lg), B, _m(START(vs)), vs, 0.0, prm)
                assert w[17] > 500 and w[18] == 131, (vs, reach, mc, w[17:21])  # 725 at 0.05 m, reach 0, min_count 3
    for name, (steps, p, m, md, prm, _) in small_scenes().items():
        A.both(cpu_table(steps, VS, md, LOG2), p, m, VS, md, prm)
    for name, (p, _) in tail_clouds().items():
        A.both(main_table(0.1, 14), p, _m(TRUTH), 0.1, 0.0, A.default_params(0.1))


def test_the_scenes_are_what_they_were_built_to_be():
    for name, (steps, p, m, md, prm, expect) in small_scenes().items():
        d = cpu_table(steps, VS, md, LOG2)
        w, keys = A.sums_py(d, p, m, VS, md, prm, detail=True)
        assert expect(w, keys.tolist()), (name, w[:21], keys)
    # the tie is a tie in every bit, and the two table orders differ
    s = small_scenes()
    da, db = cpu_table(s["tie_ab"][0], VS, 0.0, LOG2), cpu_table(s["tie_ba"][0], VS, 0.0, LOG2)
    assert np.array_equal(np.sort(da["keys"]), np.sort(db["keys"]))
    assert A.sums_np(da, s["tie_ab"][1], ident(), VS, 0.0, s["tie_ab"][4], variant="tie_largest_key", detail=True)[1][0] == A.key_of((3, 2, 8))
    # the carved voxel keeps its key with a zero payload
    d = cpu_table(s["carved_nearest"][0], VS, 0.0, LOG2)
    at = A._find(d, A.key_of((3, 2, 8)))
    assert at >= 0 and not any(int(d[n][at]) for n in ("ci", "sx", "sy", "sz"))
    # the wrapped run: homes 254, 255, 255, 254 in the slots 254, 255, 0, 1
    d = cpu_table(s["wrapped_run"][0], VS, 0.0, LOG2)
    assert [int(d["keys"][i]) for i in (254, 255, 0, 1)] == [A.key_of(c) for c in wrap_cells()]
    assert [V.fmix64(A.key_of(c)) & 255 for c in wrap_cells()] == [254, 255, 255, 254]
    # the double above D2
    assert 0.25 * 0.25 + (2.0 ** -28) * (2.0 ** -28) == np.nextafter(0.0625, 1.0)
    # the full table: no slot is free, the absent cloud shares no voxel and no neighbour with it
    p, absent = full_table()
    d = cpu_table([("insert", p, T.IDENT)], 0.1, 0.0, 8)
    assert (d["keys"] != np.uint64(V.EMPTY)).all()
    assert A.both(d, absent, T.IDENT, 0.1, 0.0, A.default_params(0.1))[17:21] == [0, 0, 130, 0]
    # the tails
    for name, (p, n_matched) in tail_clouds().items():
        assert A.sums_np(main_table(0.1, 14), p, _m(TRUTH), 0.1, 0.0, A.default_params(0.1))[17] == n_matched, name
    # the table fits and the reversed build holds the same voxels
    for vs, lg in SIZES:
        d, r = main_table(vs, lg), main_table(vs, lg, True)
        keys = d["keys"][d["keys"] != np.uint64(V.EMPTY)]
        T._fits(keys, lg)
        assert np.array_equal(np.sort(keys), np.sort(r["keys"][r["keys"] != np.uint64(V.EMPTY)]))


def test_every_misreading_of_the_contract_changes_a_stated_scene():
    B = T.second_cloud()
    d, m, prm = main_table(0.1, 14), _m(START(0.1)), A.default_params(0.1)
    base = A.sums_np(d, B, m, 0.1, 0.0, prm)
    for v in ("reach0", "first_found", "floor_no_half", "e_world", "cross_sign"):
        assert A.sums_np(d, B, m, 0.1, 0.0, prm, variant=v) != base, v
    p3 = prm._replace(min_count=3)
    assert A.sums_np(d, B, m, 0.1, 0.0, p3, variant="count_gt") != A.sums_np(d, B, m, 0.1, 0.0, p3)
    s = small_scenes()
    steps, p, mm, md, pp, _ = s["tie_ab"]
    t = cpu_table(steps, VS, md, LOG2)
    assert A.sums_np(t, p, mm, VS, md, pp, variant="tie_largest_key") != A.sums_np(t, p, mm, VS, md, pp)
    steps, p, mm, md, pp, _ = s["d2_equals_D2"]
    t = cpu_table(steps, VS, md, LOG2)
    assert A.sums_np(t, p, mm, VS, md, pp, variant="far_ge")[17:21] == [0, 0, 0, 1] and A.sums_np(t, p, mm, VS, md, pp)[17:21] == [1, 0, 0, 0]
    for name in ("half_plus", "half_minus"):
        steps, p, mm, md, pp, _ = s[name]
        t = cpu_table(steps, VS, md, LOG2)
        assert A.sums_np(t, p, mm, VS, md, pp, variant="floor_no_half")[1] == A.sums_np(t, p, mm, VS, md, pp)[1] - 1, name
    assert len(A.VARIANTS) == 8


@functools.lru_cache(maxsize=None)
def restated_loop(vs, lg, max_iters=10):
    prm = A.default_params(vs, max_iters=max_iters)
    d = main_table(vs, lg)
    return A.loop(START(vs), prm, lambda m: A.sums_np(d, T.second_cloud(), m, vs, 0.0, prm))


def test_the_loop_on_the_restatement_moves_the_displaced_cloud_towards_its_true_pose():
    for vs, lg in SIZES:
        out, res, trace = restated_loop(vs, lg)
        t0, r0 = A.pose_errors(START(vs), TRUTH)
        t1, r1 = A.pose_errors(out, TRUTH)
        assert res["status"] in ("CONVERGED", "MAX_ITERS"), (vs, res)
        assert t1 < t0 and r1 < r0, (vs, t0, t1, r0, r1)
        assert res["last_cost"] < res["first_cost"], (vs, res)
        assert abs(t0 - 0.5 * vs * math.sqrt(0.6 ** 2 + 0.5 ** 2 + 0.62 ** 2)) < 1e-9 and abs(r0 - 0.00995) < 1e-5
        assert len(trace) == res["iterations"] and trace[0][1][17] == res["first_matched"]
    # the pieces of the loop by another route: numpy's solver, and the round trip of a pose
    H, g = A.normal(restated_loop(0.1, 14)[2][0][1])
    xi = A.solve(H, g)
    assert np.allclose(np.array(H) @ np.array(xi), -np.array(g), rtol=1e-9, atol=1e-9)
    assert np.allclose(xi, np.linalg.solve(np.array(H), -np.array(g)), rtol=1e-8, atol=1e-12)
    assert A.solve([[0.0] * 6 for _ in range(6)], [0.0] * 6) is None
    u, Tt = A.from_pose7(TRUTH)
    assert np.allclose(A.to_pose7(u, Tt), TRUTH, rtol=0, atol=1e-15)
    R, m12 = A.matrix(u, Tt)
    assert np.allclose(m12, _m(TRUTH), rtol=0, atol=1e-15) and np.allclose(m12, T.MAIN_M, rtol=0, atol=1e-15)


def test_pure_entries_and_refusals_without_a_context():
    from stereo_vo_amd import api
    L = api.lib()
    for vs in (0.05, 0.1, 0.25, 3.0, 5.0):
        p, want = api.voxel_align_default_params(vs), A.default_params(vs)
        assert tuple(getattr(p, f) for f, _ in p._fields_) == tuple(F32(v) if isinstance(v, float) else v for v in want), vs
    p = api.voxel_align_default_params(5.0)
    assert p.max_dist == 8.0 and (p.min_count, p.reach, p.max_iters, p.min_matches) == (1, 1, 10, 64)
    assert api.voxel_align_default_params(0.1).max_dist == F32(0.2) and api.voxel_align_default_params(0.1).eps_r == F32(1e-5)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(api.SvoError):
            api.voxel_align_default_params(bad)
    assert L.svo_voxel_align_default_params(C.c_float(0.1), None) == -1
    buf, w = (C.c_double * 12)(), (C.c_int64 * 32)()
    prm, res = api.voxel_align_default_params(0.1), api.VoxelAlignResult()
    assert L.svo_voxel_map_align_sums_dev(None, None, 0, buf, C.byref(prm), w) == -1
    assert L.svo_voxel_map_align_sums_pose7_dev(None, None, 0, buf, C.byref(prm), w) == -1
    assert L.svo_voxel_map_align(None, None, 0, buf, C.byref(prm), buf, C.byref(res)) == -1
    assert api.VOXEL_ALIGN_STATUS == A.STATUS and api.ALIGN_COUNTS == A.COUNTS and api.VOXEL_ALIGN_WORDS == A.WORDS
    assert C.sizeof(api.VoxelAlignParams) == 28 and C.sizeof(api.VoxelAlignResult) == 88


def test_voxel_align_host_logic_under_sanitizers(tmp_path):
    """host/voxel_align.h on the CPU under ASan + UBSan: every refusal at its boundary with code and exact message and their order,
    Q_S at +-0.5/S, at the doubles next to them and at the largest magnitudes the bounds allow, the Cholesky solve on a hand-made SPD
    matrix, a singular one and one with a NaN, the pose update keeping |u| = 1 to one ulp over 10,000 random steps, the round trips
    pose7 -> (u, T) -> pose7, the loop over a functor."""
    _run_sanitized(tmp_path, "voxel_align_args_test", "voxel align args ok")


# ===================================================================================================== GPU
def _sums_buf():
    import torch
    c = torch.full((A.WORDS + 2,), SENT, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    return c


def _frozen(vm):
    return {k: v.copy() for k, v in vm.download().items()}, vm.stats()


def _call(vm, pts, prm, m12=None, pose7=None, dev=None):
    """One align_sums into a guarded buffer: the 32 words as Python ints; the guards stay; the table and the counters are untouched."""
    before, stats = _frozen(vm)
    t = T._dev(pts) if dev is None else dev
    c = _sums_buf()
    kw = dict(min_count=prm.min_count, reach=prm.reach, max_dist=prm.max_dist, max_iters=prm.max_iters, min_matches=prm.min_matches,
              eps_t=prm.eps_t, eps_r=prm.eps_r)
    vm.align_sums(t.data_ptr() if len(pts) else None, len(pts), c2w12=m12, pose7=pose7, sums_ptr=c.data_ptr() + 8, **kw)
    vm.ctx.sync()
    got = c.cpu().tolist()
    assert got[0] == SENT and got[-1] == SENT
    after, stats2 = _frozen(vm)
    assert all(np.array_equal(before[k], after[k]) for k in before) and stats2 == stats
    return got[1:-1], before


def _build(ctx, steps, vs, md, lg):
    vm = T._map(ctx, vs, lg, md)
    for kind, pts, m in steps:
        t = T._dev(pts)
        (vm.insert if kind == "insert" else vm.remove)(t.data_ptr(), len(pts), m12=m)
        vm.ctx.sync()
    return vm


@pytest.mark.gpu
@pytest.mark.parametrize("vs,lg", SIZES)
def test_main_scene_sums_by_both_entries_in_any_order(ctx, vs, lg):
    Acl, B = T.main_scene(), T.second_cloud()
    start = np.array(START(vs))
    assert restated_loop(vs, lg)[1]["first_matched"] > 1000  # the scene is what the CPU tests say it is
    for reverse_map in (False, True):
        vm = _build(ctx, [("insert", Acl[::-1] if reverse_map else Acl, _m(TRUTH))], vs, 0.0, lg)
        for reach in (0, 1):
            for mc in (1, 3):
                prm = A.default_params(vs, reach=reach, min_count=mc)
                got, d = _call(vm, B, prm, m12=_m(start))
                want = A.sums_np(d, B, _m(start), vs, 0.0, prm)
                assert got == want, (vs, reach, mc, reverse_map)
                assert want == A.sums_np(main_table(vs, lg), B, _m(start), vs, 0.0, prm)  # no slot placement matters
                assert _call(vm, B, prm, pose7=start)[0] == want
                assert _call(vm, B[::-1], prm, m12=_m(start))[0] == want
        # a repeated call, byte for byte
        prm = A.default_params(vs)
        assert _call(vm, B, prm, pose7=start)[0] == _call(vm, B, prm, pose7=start)[0]
        vm.close()


@pytest.mark.gpu
def test_wavefront_and_workgroup_tails(ctx):
    vm = _build(ctx, [("insert", T.main_scene(), _m(TRUTH))], 0.1, 0.0, 14)
    prm = A.default_params(0.1)
    for name, (p, n_matched) in tail_clouds().items():
        got, d = _call(vm, p, prm, m12=_m(TRUTH))
        assert got == A.both(d, p, _m(TRUTH), 0.1, 0.0, prm) and got[17] == n_matched, name
    # n == 0: the words are zeroed, nothing else happens
    ctx.profile_select("voxel_align")
    got, _ = _call(vm, T.main_scene()[:0], prm, m12=_m(TRUTH))
    assert ctx.profile_read()[1] == 1 and got == [0] * A.WORDS
    ctx.profile_select(None)
    vm.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(small_scenes()))
def test_constructed_records(ctx, name):
    steps, p, m, md, prm, expect = small_scenes()[name]
    vm = _build(ctx, steps, VS, md, LOG2)
    got, d = _call(vm, p, prm, m12=m)
    want, keys = A.sums_py(d, p, m, VS, md, prm, detail=True)
    assert expect(want, keys.tolist()), name  # on the table the device built
    assert got == want == A.sums_np(d, p, m, VS, md, prm), (name, got[:21], want[:21])
    if name == "wrapped_run":
        assert [int(d["keys"][i]) for i in (254, 255, 0, 1)] == [A.key_of(c) for c in wrap_cells()]
    vm.close()


@pytest.mark.gpu
def test_a_full_table_ends_every_look_up_after_64_slots(ctx):
    p, absent = full_table()
    vm = _build(ctx, [("insert", p, T.IDENT)], 0.1, 0.0, 8)
    prm = A.default_params(0.1)
    got, d = _call(vm, absent, prm, m12=T.IDENT)
    assert (d["keys"] != np.uint64(V.EMPTY)).all()
    assert got == A.both(d, absent, T.IDENT, 0.1, 0.0, prm) and got[17:21] == [0, 0, 130, 0]
    got, d = _call(vm, p, prm, m12=T.IDENT)  # what was stored is found, also behind long runs; what was dropped is absent
    assert got == A.both(d, p, T.IDENT, 0.1, 0.0, prm) and got[17] >= 256
    vm.close()


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64).tolist()


def _assert_loop(vm, pts, dev, start, prm, vs, md, want_status=None):
    """svo_voxel_map_align against the restatement's loop over the downloaded table: pose7_out and xi by bit pattern, every field
    of the result, and the device's sums at every pose the restatement went through."""
    d, _ = _frozen(vm)
    out, res, trace = A.loop(start, prm, lambda m: A.sums_np(d, pts, m, vs, md, prm))
    got_out, got = vm.align(dev.data_ptr(), len(pts), np.array(start), **prm._asdict())
    assert _bits(got_out) == _bits(out), (got_out, out)
    assert _bits(got["xi"]) == _bits(res["xi"])
    assert {k: v for k, v in got.items() if k != "xi"} == {k: v for k, v in res.items() if k != "xi"}, (got, res)
    for m12, words in trace:
        assert _call(vm, pts, prm, m12=np.array(m12), dev=dev)[0] == words
    if want_status is not None:
        assert res["status"] == want_status, res
    return out, res


@pytest.mark.gpu
@pytest.mark.parametrize("vs,lg", SIZES)
def test_the_loop_equals_the_restatement_in_every_bit(ctx, vs, lg):
    B = T.second_cloud()
    vm = _build(ctx, [("insert", T.main_scene(), _m(TRUTH))], vs, 0.0, lg)
    dev = T._dev(B)
    prm = A.default_params(vs)
    ctx.profile_select("voxel_align")
    out, res = _assert_loop(vm, B, dev, START(vs), prm, vs, 0.0)
    assert ctx.profile_read()[1] == 2 * res["iterations"]  # the loop's launches, and the sums asked for again pose by pose
    ctx.profile_select(None)
    want_out, want_res, _ = restated_loop(vs, lg)  # the CPU test's run: no slot placement matters
    assert _bits(out) == _bits(want_out) and res == want_res
    # one iteration: a step is taken and the status says that the bound ended it
    out1, res1 = _assert_loop(vm, B, dev, START(vs), prm._replace(max_iters=1), vs, 0.0, "MAX_ITERS")
    assert res1["iterations"] == 1 and _bits(out1) != _bits(START(vs))
    vm.close()


@pytest.mark.gpu
def test_the_loop_ends_with_too_few_and_degenerate(ctx):
    vs = 0.1
    B = T.second_cloud()
    vm = _build(ctx, [("insert", T.main_scene(), _m(TRUTH))], vs, 0.0, 14)
    dev = T._dev(B)
    far = A.displaced(TRUTH, [500.0, 0.0, 0.0], [0.0, 0.0, 0.0])
    out, res = _assert_loop(vm, B, dev, far, A.default_params(vs), vs, 0.0, "TOO_FEW")
    assert res["iterations"] == 1 and res["first_matched"] == 0 and _bits(out) == _bits(far)  # no step: the input pose, bit for bit
    _assert_loop(vm, B[:0], dev, START(vs), A.default_params(vs), vs, 0.0, "TOO_FEW")  # n == 0
    vm.close()
    # all matched points on one line (the camera's axis): the rotation about it is free and the last pivot is exactly 0
    line = V.records(np.zeros(8, F32), np.zeros(8, F32), (1.0 + 0.37 * np.arange(8)).astype(F32), np.arange(8, dtype=np.uint32))
    vm = _build(ctx, [("insert", line, T.IDENT)], vs, 0.0, 8)
    pose = [1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    out, res = _assert_loop(vm, line, T._dev(line), pose, A.default_params(vs, min_matches=6), vs, 0.0, "DEGENERATE")
    assert res["first_matched"] == 8 and res["iterations"] == 1 and _bits(out) == _bits(pose)
    vm.close()


@pytest.mark.gpu
def test_bad_arguments_launch_nothing_and_leave_the_map_usable(ctx):
    from stereo_vo_amd import api
    L = ctx.L
    vs = 0.1
    B = T.second_cloud()
    vm = _build(ctx, [("insert", T.main_scene(), _m(TRUTH))], vs, 0.0, 14)
    t, c = T._dev(B), _sums_buf()
    m = np.ascontiguousarray(_m(TRUTH))
    mp = m.ctypes.data_as(C.c_void_p)
    q = (C.c_double * 7)(*TRUTH)
    out = (C.c_double * 7)(*([7.0] * 7))
    res = api.VoxelAlignResult()
    res.status, res.iterations = 77, 77
    ok = api.voxel_align_default_params(vs)

    def P(**kw):
        return C.byref(api._params(lambda: api.voxel_align_default_params(vs), None, **kw))

    sums = lambda n=5, pts=None, mat=mp, prm=C.byref(ok), s=None: L.svo_voxel_map_align_sums_dev(
        vm.h, t.data_ptr() if pts is None else pts, n, mat, prm, c.data_ptr() + 8 if s is None else s)
    calls = [(lambda: sums(n=-1), "n must not"), (lambda: sums(n=(1 << 20) + 1), "2^20"), (lambda: sums(mat=None), "c2w12"),
             (lambda: sums(prm=None), "params"), (lambda: sums(prm=P(min_count=0)), "min_count"), (lambda: sums(prm=P(reach=2)), "reach"),
             (lambda: sums(prm=P(reach=-1)), "reach"), (lambda: sums(prm=P(max_dist=0.0)), "max_dist"),
             (lambda: sums(prm=P(max_dist=8.5)), "max_dist"), (lambda: sums(prm=P(max_dist=float("nan"))), "max_dist"),
             (lambda: sums(prm=P(max_dist=float("inf"))), "max_dist"), (lambda: sums(prm=P(max_iters=0)), "max_iters"),
             (lambda: sums(prm=P(min_matches=5)), "min_matches"), (lambda: sums(prm=P(eps_t=-1.0)), "eps_t"),
             (lambda: sums(prm=P(eps_t=float("inf"))), "eps_t"), (lambda: sums(prm=P(eps_r=float("nan"))), "eps_r"),
             (lambda: sums(s=0), "sums"), (lambda: sums(s=c.data_ptr() + 12), "8-byte"), (lambda: sums(pts=0), "points"),
             (lambda: sums(pts=t.data_ptr() + 2), "4-byte"),
             (lambda: L.svo_voxel_map_align_sums_pose7_dev(vm.h, t.data_ptr(), 5, None, C.byref(ok), c.data_ptr() + 8), "pose7"),
             (lambda: L.svo_voxel_map_align(vm.h, t.data_ptr(), -1, q, C.byref(ok), out, C.byref(res)), "n must not"),
             (lambda: L.svo_voxel_map_align(vm.h, t.data_ptr(), 5, None, C.byref(ok), out, C.byref(res)), "pose7_in"),
             (lambda: L.svo_voxel_map_align(vm.h, t.data_ptr(), 5, q, C.byref(ok), None, C.byref(res)), "pose7_out"),
             (lambda: L.svo_voxel_map_align(vm.h, t.data_ptr(), 5, q, C.byref(ok), out, None), "result"),
             (lambda: L.svo_voxel_map_align(vm.h, t.data_ptr(), 5, q, None, out, C.byref(res)), "params"),
             (lambda: L.svo_voxel_map_align(vm.h, t.data_ptr(), 5, q, P(max_iters=0), out, C.byref(res)), "max_iters"),
             (lambda: L.svo_voxel_map_align(vm.h, None, 5, q, C.byref(ok), out, C.byref(res)), "points"),
             (lambda: L.svo_voxel_map_align(vm.h, t.data_ptr() + 1, 5, q, C.byref(ok), out, C.byref(res)), "4-byte")]
    before, stats = _frozen(vm)
    ctx.profile_select("voxel_align")
    for call, word in calls:
        assert call() == -1 and word in L.svo_last_error(ctx.h).decode(), (word, L.svo_last_error(ctx.h).decode())
    assert ctx.profile_read()[1] == 0
    ctx.profile_select(None)
    ctx.sync()
    assert c.cpu().tolist() == [SENT] * (A.WORDS + 2) and list(out) == [7.0] * 7 and (res.status, res.iterations) == (77, 77)
    after, stats2 = _frozen(vm)
    assert all(np.array_equal(before[k], after[k]) for k in before) and stats2 == stats
    with pytest.raises(ValueError):
        vm.align_sums(t.data_ptr(), 5, sums_ptr=c.data_ptr() + 8)
    # the context and the map work
    prm = A.default_params(vs)
    got, d = _call(vm, B, prm, pose7=np.array(TRUTH))
    assert got == A.sums_np(d, B, _m(TRUTH), vs, 0.0, prm)
    vm.close()
