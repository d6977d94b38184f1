"""The voxel map normals and the plane form of the align (include/svo.h, "Voxel map normals", "Voxel map align, plane form"; DESIGN
7r) against the restatement tests/voxel_normals_ref.py: floats by bit pattern, integers with ==.

CPU: the restatement's two routes agree on every scene, for normals and for sums; each deliberate misreading of the contract changes
a stated scene; the constructed scenes are what they were built to be; the pure entries and the refusals that need no context;
host/voxel_normals.h and host/voxel_align_plane.h under ASan + UBSan (tests/sanitize/voxel_normals_args_test.cpp); the plane loop on
the restatement alone.
GPU: every record of the side array and all eight counts, into sentinel-filled guarded buffers, equal the restatement run on the
DOWNLOADED table; the 40 words of the plane sums likewise; svo_voxel_map_align_plane equals the restatement's loop in every bit; the
table's bytes and the map's counters are unchanged after every call.

The corner scene (voxel_normals_ref.corner_scene: a floor, a back wall and a side wall, 12,800 records, z from 2.33 to 5.11; seed 10
is the map's cloud, seed 11 the aligned one, both under test_voxel_align.TRUTH) holds 8,052 / 2,702 / 449 voxels at 0.05 / 0.1 /
0.25 m; at the defaults 7,663 / 2,699 / 449 get a normal and 389 / 3 / 0 have fewer than five neighbours; max_curvature 0.05 refuses
3,739 / 320 / 73 more.  From test_voxel_align.START(vs), ten iterations at the defaults, on the restatement (translation error in map
units, rotation error in radians):
  voxel    start              point-to-mean loop     plane loop
  0.05 m   0.02493 0.00995    0.00316 0.00380        0.00140 0.00049   MAX_ITERS
  0.1 m    0.04986 0.00995    0.00423 0.00585        0.00217 0.00078   CONVERGED after 7
  0.25 m   0.12465 0.00995    0.02136 0.01053        0.00804 0.00287   CONVERGED after 6
On the two-plane scene of tests/test_voxel_map.py the shift along the planes' common line is free: the rotation error falls to 0.00174 /
0.00246 / 0.00183 and the cost falls, the translation error goes 0.02493 -> 0.03214, 0.04986 -> 0.05554, 0.12465 -> 0.03949.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import voxel_align_ref as A
import voxel_normals_ref as N
import voxel_ref as V
import test_voxel_align as TA
import test_voxel_map as T
from test_host_sanitizers import _run_sanitized

SIZES = TA.SIZES
TRUTH, START, VS, LOG2, SENT = TA.TRUTH, TA.START, TA.VS, TA.LOG2, TA.SENT
SENT32 = 0x5A5A5A5A
NONE_BITS = (0, 0, 0, 0xBF800000)
ONE = 0x3F800000
K = A.key_of
LO, HI = -(1 << 20), (1 << 20) - 1  # the ends of the key range


@functools.lru_cache(maxsize=None)
def corner(seed):
    p = N.corner_scene(seed=seed)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def corner_table(vs, lg, reverse=False):
    a = corner(10)
    return TA.cpu_table([("insert", a[::-1] if reverse else a, TA._m(TRUTH))], vs, 0.0, lg)


@functools.lru_cache(maxsize=None)
def corner_normals(vs, lg, min_count=1, max_curvature=1.0):
    return N.normals_np(corner_table(vs, lg), N.default_params(min_count=min_count, max_curvature=max_curvature))


def at_x(cells, x_index, frac=(0.5, 0.5, 0.5)):
    """One record per cell whose x index is moved to x_index + (the cell's x) by the matrix: (records, m12)."""
    return TA.cat(*[TA.rec(c, frac) for c in cells]), TA.ident((float(x_index) * VS, 0.0, 0.0))


@functools.lru_cache(maxsize=None)
def small_scenes():
    """name -> (steps, params, expectation(key -> record bits, counts)) at VS in a 2^8 table; the fractions are dyadic."""
    P = N.default_params
    out = {}
    grid = [(a, b) for a in (2, 3, 4) for b in (2, 3, 4)]
    # nine voxels in a plane along each axis, equal fractions: the centre's normal is the axis, its curvature 0; the four corners
    # have four participants
    for name, cells, centre, want in (("plane_z", [(a, b, 8) for a, b in grid], (3, 3, 8), (0, 0, ONE, 0)),
                                      ("plane_y", [(a, 3, 6 + b) for a, b in grid], (3, 3, 9), (0, ONE, 0, 0)),
                                      ("plane_x", [(3, a, 6 + b) for a, b in grid], (3, 3, 9), (ONE, 0, 0, 0))):
        steps = [("insert", TA.cat(*[TA.rec(c) for c in cells]), TA.ident())]
        out[name] = (steps, P(), lambda r, c, centre=centre, want=want: r[K(centre)] == want and c[:5] == [9, 5, 4, 0, 0] and
                     sorted(set(r.values())) == sorted({want, NONE_BITS}))
    # slabs about x + y = const and x - y = const, three layers in z, the y fractions mirroring the x fractions: |nx| == |ny| in every bit;
    # the largest magnitude's LOWEST index is made positive, so x - y gives (+, -, 0)
    fr = {-1: 0.25, 0: 0.5, 1: 0.625}
    for name, sy in (("plane_x_plus_y", -1), ("plane_x_minus_y", 1)):
        recs = [TA.rec((3 + t, 3 + sy * t, 8 + l), (fr[t], fr[sy * t] if sy == 1 else fr[-t], 0.5)) for t in (-1, 0, 1) for l in (-1, 0, 1)]
        def expect(r, c, sy=sy):
            nx, ny, nz, cu = r[K((3, 3, 8))]
            return nx & 0x7FFFFFFF == ny & 0x7FFFFFFF and nx >> 31 == 0 and ny >> 31 == (1 if sy == 1 else 0) and nz & 0x7FFFFFFF == 0 and cu < 0x3B000000  # curvature below 2^-9
        out[name] = ([("insert", TA.cat(*recs), TA.ident())], P(), expect)
    # three and five voxels on a line: the inner ones are collinear, the ends have two participants
    for name, n in (("collinear_3", 3), ("collinear_5", 5)):
        steps = [("insert", TA.cat(*[TA.rec((2 + i, 3, 8), (0.25, 0.5, 0.75)) for i in range(n)]), TA.ident())]
        out[name] = (steps, P(min_neighbours=3), lambda r, c, n=n: c[:5] == [n, 0, 2, n - 2, 0] and set(r.values()) == {NONE_BITS})
    # the centre and three neighbours against min_neighbours 5, and one more
    four = [(3, 3, 8), (4, 3, 8), (3, 4, 8), (2, 2, 8)]
    out["four_participants"] = ([("insert", TA.cat(*[TA.rec(c) for c in four]), TA.ident())], P(), lambda r, c: c[:5] == [4, 0, 4, 0, 0])
    out["five_participants"] = ([("insert", TA.cat(*[TA.rec(c) for c in four + [(4, 4, 8)]]), TA.ident())], P(),
                                lambda r, c: r[K((3, 3, 8))] == (0, 0, ONE, 0) and c[1] >= 1)
    # a neighbour below min_count takes no part and is no centre: with it the plane would have a thickness
    recs = [TA.rec(c) for c in [(a, b, 8) for a, b in grid]] * 2 + [TA.rec((3, 3, 9), (0.5, 0.5, 0.25))]
    out["neighbour_below_min_count"] = ([("insert", TA.cat(*recs), TA.ident())], P(min_count=2),
                                        lambda r, c: r[K((3, 3, 8))] == (0, 0, ONE, 0) and r[K((3, 3, 9))] == NONE_BITS and c[0] == 9)
    out["neighbour_at_min_count"] = ([("insert", TA.cat(*recs), TA.ident())], P(min_count=1),
                                     lambda r, c: r[K((3, 3, 8))] not in ((0, 0, ONE, 0), NONE_BITS) and c[0] == 10)
    # a carved neighbour (a removal's emptied voxel: the key stays, the count is 0)
    steps = [("insert", TA.cat(*recs), TA.ident()), ("remove", recs[-1], TA.ident())]
    out["carved_neighbour"] = (steps, P(), lambda r, c: r[K((3, 3, 8))] == (0, 0, ONE, 0) and r[K((3, 3, 9))] == NONE_BITS and c[0] == 9)
    # centres at both ends of the key range: a candidate whose index leaves it has no key.  Formed all the same, its key would be the
    # key of a voxel at the OTHER end (the field wraps into its neighbour), and that voxel is here, at another height inside its voxel
    low, m_low = at_x([(a, b, 8) for a in (0, 1) for b in (2, 3, 4)], LO)
    high, m_high = at_x([(a, b, 8) for a in (-1, 0) for b in (1, 2, 3, 4, 5)], HI, (0.5, 0.5, 0.75))
    def expect_ends(r, c):
        return r[K((LO, 3, 8))] == (0, 0, ONE, 0) and r[K((HI, 3, 8))] == (0, 0, ONE, 0) and c[0] == 16
    out["ends_of_the_key_range"] = ([("insert", low, m_low), ("insert", high, m_high)], P(), expect_ends)
    # lambda = (4, 4, 8) k: curvature exactly 0.25 against max_curvature 0.25, and the tie of the two smallest goes to index 0
    cells = [(3, 3, 8)] + [(3 + a, 3, 8 + b) for a in (-1, 1) for b in (-1, 1)] + [(3, 3 + a, 8 + b) for a in (-1, 1) for b in (-1, 1)]
    out["curvature_at_the_bound"] = ([("insert", TA.cat(*[TA.rec(c) for c in cells]), TA.ident())], P(max_curvature=0.25),
                                     lambda r, c: r[K((3, 3, 8))] == (ONE, 0, 0, 0x3E800000))
    return out


@functools.lru_cache(maxsize=None)
def full_table():
    """3,000 distinct voxels at 0.1 m into 2^8 slots (tests/test_voxel_align.py): every slot is taken, every absent neighbour costs
    64 probes."""
    p, _ = TA.full_table()
    return TA.cpu_table([("insert", p, T.IDENT)], 0.1, 0.0, 8)


def one_plane(n=12):
    """n x n voxels in the plane z = 8 at VS, one record each: every normal is (0, 0, 1) or none."""
    return TA.cat(*[TA.rec((a - 6, b - 6, 8), (0.5, 0.25, 0.5)) for a in range(n) for b in range(n)])


# ===================================================================================================== CPU
def test_the_two_routes_of_the_restatement_agree_on_every_scene():
    B = corner(11)
    for vs, lg in SIZES:
        for mc in (1, 3):
            for cu in (1.0, 0.05):
                _, c = N.both(corner_table(vs, lg), N.default_params(min_count=mc, max_curvature=cu))
                assert c[1] > 50, (vs, mc, cu, c)
        nrm, _ = corner_normals(vs, lg)
        w = N.plane_both(corner_table(vs, lg), nrm, B, TA._m(START(vs)), vs, 0.0, A.default_params(vs))
        assert w[29] > 12000, (vs, w[29:34])
    nrm, _ = corner_normals(0.1, 14, 1, 0.05)
    for reach, mc in ((0, 1), (1, 3)):
        w = N.plane_both(corner_table(0.1, 14), nrm, B, TA._m(START(0.1)), 0.1, 0.0, A.default_params(0.1, reach=reach, min_count=mc))
        assert w[29] > 3000 and w[33] > 300, (reach, mc, w[29:34])
    for name, (steps, prm, _) in small_scenes().items():
        N.both(TA.cpu_table(steps, VS, 0.0, LOG2), prm)
    N.both(full_table(), N.default_params())


def test_the_scenes_are_what_they_were_built_to_be():
    want = {0.05: (8052, 7663, 389, 3739, 30), 0.1: (2702, 2699, 3, 320, 7), 0.25: (449, 449, 0, 73, 3)}
    a = corner(10)
    assert len(a) == 12800 and abs(float(a["z"].min()) - 2.33) < 0.005 and abs(float(a["z"].max()) - 5.11) < 0.005
    for vs, lg in SIZES:
        d = corner_table(vs, lg)
        occ = d["keys"] != np.uint64(V.EMPTY)
        c, c5 = corner_normals(vs, lg)[1], corner_normals(vs, lg, 1, 0.05)[1]
        assert (int(occ.sum()), c[1], c[2], c5[4], V.longest_run(occ)) == want[vs], vs
        assert c[:5] == [want[vs][0], want[vs][1], want[vs][2], 0, 0] and c5[2] == c[2]
        r = corner_table(vs, lg, True)
        assert np.array_equal(np.sort(d["keys"]), np.sort(r["keys"]))
        assert N.by_key(d, corner_normals(vs, lg)[0]) == N.by_key(r, N.normals_np(r, N.default_params())[0])  # no slot placement matters
    for name, (steps, prm, expect) in small_scenes().items():
        d = TA.cpu_table(steps, VS, 0.0, LOG2)
        nrm, c = N.normals_py(d, prm)
        assert expect(N.by_key(d, nrm), c), (name, c, N.by_key(d, nrm))
    # the ends of the key range: the keys a wrapping field would form are keys of the table
    d = TA.cpu_table(small_scenes()["ends_of_the_key_range"][0], VS, 0.0, LOG2)
    keys = set(d["keys"].tolist())
    assert K((LO, 3, 8)) - 1 == K((HI, 2, 8)) and K((HI, 2, 8)) in keys and K((HI, 3, 8)) + 1 == K((LO, 4, 8)) and K((LO, 4, 8)) in keys
    # the full table: no slot is free
    assert (full_table()["keys"] != np.uint64(V.EMPTY)).all() and N.normals_np(full_table(), N.default_params())[1][1] > 50
    # a valid normal is never all zero, and has unit length to f32's rounding
    nrm, c = corner_normals(0.1, 14)
    valid = nrm["curvature"] >= 0
    assert int(valid.sum()) == c[1]
    n2 = nrm["nx"].astype(np.float64) ** 2 + nrm["ny"].astype(np.float64) ** 2 + nrm["nz"].astype(np.float64) ** 2
    assert np.abs(n2[valid] - 1.0).max() < 1e-6 and (n2[~valid] == 0).all() and float(nrm["curvature"][valid].max()) <= 1 / 3 + 1e-7


def test_every_misreading_of_the_contract_changes_a_stated_scene():
    d = corner_table(0.1, 14)
    prm = N.default_params()
    base = N.bits(N.normals_np(d, prm)[0])
    for v in ("count_weighted", "no_factor_n", "float_mean", "three_sweeps", "no_centre"):
        assert not np.array_equal(N.bits(N.normals_np(d, prm, variant=v)[0]), base), v
    fine = corner_table(0.05, 14)  # at 0.1 m the Jacobi's own column already has its largest component positive everywhere
    assert not np.array_equal(N.bits(N.normals_np(fine, prm, variant="no_sign_rule")[0]), N.bits(corner_normals(0.05, 14)[0]))
    steps, p, _ = small_scenes()["curvature_at_the_bound"]
    t = TA.cpu_table(steps, VS, 0.0, LOG2)
    assert N.normals_np(t, p)[1][:5] == [9, 1, 8, 0, 0] and N.normals_np(t, p, variant="curv_lt")[1][:5] == [9, 0, 8, 0, 1]
    assert len(N.VARIANTS) == 7
    # the sums: normals at max_curvature 0.05, so that many matched voxels have none
    nrm, _ = corner_normals(0.1, 14, 1, 0.05)
    B, m, ap = corner(11), TA._m(START(0.1)), A.default_params(0.1)
    base = N.plane_sums_np(d, nrm, B, m, 0.1, 0.0, ap)
    assert base[33] > 300
    for v in N.PLANE_VARIANTS:
        assert N.plane_sums_np(d, nrm, B, m, 0.1, 0.0, ap, variant=v) != base, v
    assert N.plane_sums_np(d, nrm, B, m, 0.1, 0.0, ap, variant="nearest_with_normal")[33] == 0
    assert len(N.PLANE_VARIANTS) == 4


def test_pure_entries_and_refusals_without_a_context():
    from stereo_vo_amd import api
    L = api.lib()
    p = api.voxel_normals_default_params()
    assert (p.min_count, p.min_neighbours, p.max_curvature) == tuple(N.default_params()) == (1, 5, 1.0)
    assert L.svo_voxel_normals_default_params(None) == -1
    for lg in (8, 14, 28):
        mp = api.VoxelMapParams(0.1, lg, 0.0)
        assert api.voxel_map_normals_bytes(mp) == 16 << lg and 5 * api.voxel_map_normals_bytes(mp) == 2 * api.voxel_map_bytes(mp)
    for bad in (api.VoxelMapParams(0.1, 7, 0.0), api.VoxelMapParams(0.1, 29, 0.0), api.VoxelMapParams(0.0, 14, 0.0), api.VoxelMapParams(float("nan"), 14, 0.0)):
        with pytest.raises(api.SvoError):
            api.voxel_map_normals_bytes(bad)
    n = C.c_size_t(7)
    assert L.svo_voxel_map_normals_bytes(None, C.byref(n)) == -1 and n.value == 0 and L.svo_voxel_map_normals_bytes(C.byref(mp), None) == -1
    buf, w = (C.c_double * 12)(), (C.c_int64 * 40)()
    ap, res = api.voxel_align_default_params(0.1), api.VoxelAlignResult()
    assert L.svo_voxel_map_normals_dev(None, C.byref(p), buf, None) == -1 and L.svo_voxel_map_normals(None, C.byref(p), buf, None) == -1
    assert L.svo_voxel_map_align_plane_sums_dev(None, buf, None, 0, buf, C.byref(ap), w) == -1
    assert L.svo_voxel_map_align_plane_sums_pose7_dev(None, buf, None, 0, buf, C.byref(ap), w) == -1
    assert L.svo_voxel_map_align_plane(None, buf, None, 0, buf, C.byref(ap), buf, C.byref(res)) == -1
    assert C.sizeof(api.VoxelNormalsParams) == 12 and api.VoxelNormal.itemsize == 16 and api.VoxelNormal == N.NORMAL
    assert api.NORMALS_COUNTS == N.COUNTS and api.VOXEL_NORMALS_COUNTS == N.N_COUNTS
    assert api.VOXEL_ALIGN_PLANE_WORDS == N.PLANE_WORDS and api.ALIGN_PLANE_COUNTS == N.PLANE_COUNTS
    assert [N.word_of(i, k) for i in range(6) for k in range(i, 6)] == list(range(1, 22))


def test_voxel_normals_host_logic_under_sanitizers(tmp_path):
    """host/voxel_normals.h and host/voxel_align_plane.h on the CPU under ASan + UBSan: every refusal at its boundary with code, exact
    message and order, the defaults and sizes, the moments and the Jacobi on neighbourhoods whose records the Python restatement
    gave bit for bit, on 20,000 random and on degenerate ones, H and g from 40 words, a match's terms against a long double
    restatement, and a few thousand loop steps on words summed from three synthetic planes (one plane ends DEGENERATE)."""
    _run_sanitized(tmp_path, "voxel_normals_args_test", "voxel normals args ok")


@functools.lru_cache(maxsize=None)
def restated_plane_loop(vs, lg):
    prm = A.default_params(vs)
    d, nrm = corner_table(vs, lg), corner_normals(vs, lg)[0]
    return N.plane_loop(START(vs), prm, lambda m: N.plane_sums_np(d, nrm, corner(11), m, vs, 0.0, prm))


def test_the_plane_loop_on_the_restatement_beats_the_point_loop_on_the_corner_scene():
    for vs, lg in SIZES:
        out, res, trace = restated_plane_loop(vs, lg)
        prm = A.default_params(vs)
        d = corner_table(vs, lg)
        point, _, _ = A.loop(START(vs), prm, lambda m: A.sums_np(d, corner(11), m, vs, 0.0, prm))
        (t0, r0), (t1, r1), (tp, rp) = A.pose_errors(START(vs), TRUTH), A.pose_errors(out, TRUTH), A.pose_errors(point, TRUTH)
        print(f"corner {vs}: start {t0:.5f} {r0:.5f}  point {tp:.5f} {rp:.5f}  plane {t1:.5f} {r1:.5f}  {res['status']} {res['iterations']}")
        assert res["status"] in ("CONVERGED", "MAX_ITERS"), (vs, res)
        assert t1 < t0 and r1 < r0 and res["last_cost"] < res["first_cost"], (vs, t0, t1, r0, r1, res)
        assert t1 < tp and r1 < rp, (vs, t1, tp, r1, rp)
        assert len(trace) == res["iterations"] and trace[0][1][29] == res["first_matched"]
    # H from the words by another route: numpy's solver on the first iteration's system
    H, g = N.plane_normal(restated_plane_loop(0.1, 14)[2][0][1])
    xi = A.solve(H, g)
    assert np.allclose(np.array(H), np.array(H).T, rtol=0, atol=0) and np.allclose(xi, np.linalg.solve(np.array(H), -np.array(g)), rtol=1e-7, atol=1e-12)


def test_the_plane_loop_on_the_two_plane_scene_turns_the_cloud_and_lowers_the_cost():
    for vs, lg in SIZES:
        d = TA.main_table(vs, lg)
        nrm, _ = N.normals_np(d, N.default_params())
        prm = A.default_params(vs)
        out, res, _ = N.plane_loop(START(vs), prm, lambda m: N.plane_sums_np(d, nrm, T.second_cloud(), m, vs, 0.0, prm))
        (t0, r0), (t1, r1) = A.pose_errors(START(vs), TRUTH), A.pose_errors(out, TRUTH)
        print(f"two-plane {vs}: start {t0:.5f} {r0:.5f}  plane {t1:.5f} {r1:.5f}  {res['status']} {res['iterations']}")
        assert r1 < r0 and res["last_cost"] < res["first_cost"], (vs, r0, r1, res)  # the shift along the common line is free


# ===================================================================================================== GPU
def _normals_call(vm, prm, with_counts=True):
    """One normals launch into guarded buffers: (the records by slot, the 8 counts or None, the downloaded table)."""
    import torch
    before, stats = TA._frozen(vm)
    cap = vm.capacity
    buf = torch.full(((cap + 2) * 4,), SENT32, dtype=torch.int32, device="cuda")  # one guard record on each side
    cnt = torch.full((N.N_COUNTS + 2,), SENT, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    vm.normals(buf.data_ptr() + 16, counts_ptr=cnt.data_ptr() + 8 if with_counts else None, **prm._asdict())
    vm.ctx.sync()
    raw, c = buf.cpu().numpy().view(np.uint32), cnt.cpu().tolist()
    assert (raw[:4] == SENT32).all() and (raw[-4:] == SENT32).all() and c[0] == SENT and c[-1] == SENT
    if not with_counts:
        assert c == [SENT] * (N.N_COUNTS + 2)
    after, stats2 = TA._frozen(vm)
    assert all(np.array_equal(before[k], after[k]) for k in before) and stats2 == stats
    return raw[4:-4].copy().view(N.NORMAL), (c[1:-1] if with_counts else None), before, buf


def _assert_normals(vm, prm):
    got, c, d, buf = _normals_call(vm, prm)
    want, wc = N.normals_np(d, prm)
    bad = np.flatnonzero((N.bits(got) != N.bits(want)).any(axis=1))
    assert not len(bad), (len(bad), bad[:4], got[bad[:4]], want[bad[:4]])
    assert c == wc, (c, wc)
    return got, c, d, buf


@pytest.mark.gpu
@pytest.mark.parametrize("vs,lg", SIZES)
def test_corner_scene_normals_in_either_table_order(ctx, vs, lg):
    a = corner(10)
    by_key = {}
    for reverse in (False, True):
        vm = TA._build(ctx, [("insert", a[::-1] if reverse else a, TA._m(TRUTH))], vs, 0.0, lg)
        for mc in (1, 3):
            for cu in (1.0, 0.05):
                prm = N.default_params(min_count=mc, max_curvature=cu)
                got, c, d, _ = _assert_normals(vm, prm)
                assert by_key.setdefault((mc, cu), N.by_key(d, got)) == N.by_key(d, got)  # per key: the slot of a key is not defined
        assert c[0] > 100 and by_key[(1, 1.0)] == N.by_key(corner_table(vs, lg), corner_normals(vs, lg)[0])
        # the synchronous entry, the launch without counts, and a repeated call byte for byte
        host, hc = vm.normals_host(**N.default_params()._asdict())
        got, c, d, _ = _assert_normals(vm, N.default_params())
        assert np.array_equal(N.bits(host), N.bits(got)) and [hc[k] for k in N.COUNTS] == c[:5]
        assert np.array_equal(N.bits(_normals_call(vm, N.default_params(), with_counts=False)[0]), N.bits(got))
        vm.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(small_scenes()))
def test_constructed_neighbourhoods(ctx, name):
    steps, prm, expect = small_scenes()[name]
    vm = TA._build(ctx, steps, VS, 0.0, LOG2)
    got, c, d, _ = _assert_normals(vm, prm)
    assert expect(N.by_key(d, got), c), (name, c)
    want, wc = N.normals_py(d, prm)
    assert np.array_equal(N.bits(got), N.bits(want)) and c == wc
    vm.close()


@pytest.mark.gpu
def test_normals_of_a_full_table_and_the_profile_bracket(ctx):
    p, _ = TA.full_table()
    vm = TA._build(ctx, [("insert", p, T.IDENT)], 0.1, 0.0, 8)
    ctx.profile_select("voxel_normals")
    got, c, d, _ = _assert_normals(vm, N.default_params())
    assert ctx.profile_read()[1] == 1
    ctx.profile_select(None)
    assert (d["keys"] != np.uint64(V.EMPTY)).all() and c[0] == 256 and c[1] > 50
    want, wc = N.normals_py(d, N.default_params())
    assert np.array_equal(N.bits(got), N.bits(want)) and c == wc
    vm.close()


def _plane_call(vm, nptr, pts, prm, m12=None, pose7=None, dev=None):
    """One align_plane_sums into a guarded buffer: the 40 words as Python ints; the table and the counters are untouched."""
    import torch
    before, stats = TA._frozen(vm)
    t = T._dev(pts) if dev is None else dev
    c = torch.full((N.PLANE_WORDS + 2,), SENT, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    vm.align_plane_sums(nptr, t.data_ptr() if len(pts) else None, len(pts), c2w12=m12, pose7=pose7, sums_ptr=c.data_ptr() + 8, **prm._asdict())
    vm.ctx.sync()
    got = c.cpu().tolist()
    assert got[0] == SENT and got[-1] == SENT
    after, stats2 = TA._frozen(vm)
    assert all(np.array_equal(before[k], after[k]) for k in before) and stats2 == stats
    return got[1:-1]


@pytest.mark.gpu
@pytest.mark.parametrize("vs,lg", SIZES)
def test_corner_scene_plane_sums_by_both_entries_in_any_order(ctx, vs, lg):
    B = corner(11)
    start = np.array(START(vs))
    vm = TA._build(ctx, [("insert", corner(10), TA._m(TRUTH))], vs, 0.0, lg)
    for cu in (1.0, 0.05):
        nrm, _, d, buf = _assert_normals(vm, N.default_params(max_curvature=cu))
        nptr = buf.data_ptr() + 16
        for reach, mc in ((1, 1), (0, 1), (1, 3)):
            prm = A.default_params(vs, reach=reach, min_count=mc)
            want = N.plane_sums_np(d, nrm, B, TA._m(start), vs, 0.0, prm)
            assert _plane_call(vm, nptr, B, prm, m12=TA._m(start)) == want, (vs, cu, reach, mc)
            assert sum(want[29:34]) == len(B) and want[0] == want[29] > 500 and (cu == 1.0 or want[33] > 50)
        prm = A.default_params(vs)
        want = N.plane_sums_np(d, nrm, B, TA._m(start), vs, 0.0, prm)
        assert want == N.plane_sums_np(corner_table(vs, lg), corner_normals(vs, lg, 1, cu)[0], B, TA._m(start), vs, 0.0, prm)  # no slot placement matters
        assert _plane_call(vm, nptr, B, prm, pose7=start) == want
        assert _plane_call(vm, nptr, B[::-1], prm, m12=TA._m(start)) == want
        assert _plane_call(vm, nptr, B[:257], prm, pose7=start) == N.plane_both(d, nrm, B[:257], TA._m(start), vs, 0.0, prm)  # a workgroup and one record
    # n == 0: the words are zeroed, nothing else happens
    ctx.profile_select("voxel_align_plane")
    assert _plane_call(vm, nptr, B[:0], prm, m12=TA._m(start)) == [0] * N.PLANE_WORDS and ctx.profile_read()[1] == 1
    ctx.profile_select(None)
    vm.close()


def _assert_plane_loop(vm, nrm, nptr, pts, dev, start, prm, vs, want_status=None):
    """svo_voxel_map_align_plane against the restatement's loop over the downloaded table and normals: pose7_out and xi by bit
    pattern, every field of the result, and the device's sums at every pose the restatement went through."""
    d, _ = TA._frozen(vm)
    out, res, trace = N.plane_loop(start, prm, lambda m: N.plane_sums_np(d, nrm, pts, m, vs, 0.0, prm))
    got_out, got = vm.align_plane(nptr, dev.data_ptr(), len(pts), np.array(start), **prm._asdict())
    assert TA._bits(got_out) == TA._bits(out), (got_out, out)
    assert TA._bits(got["xi"]) == TA._bits(res["xi"])
    assert {k: v for k, v in got.items() if k != "xi"} == {k: v for k, v in res.items() if k != "xi"}, (got, res)
    for m12, words in trace:
        assert _plane_call(vm, nptr, pts, prm, m12=np.array(m12), dev=dev) == words
    if want_status is not None:
        assert res["status"] == want_status, res
    return out, res


@pytest.mark.gpu
@pytest.mark.parametrize("vs,lg", SIZES)
def test_the_plane_loop_equals_the_restatement_in_every_bit(ctx, vs, lg):
    B = corner(11)
    vm = TA._build(ctx, [("insert", corner(10), TA._m(TRUTH))], vs, 0.0, lg)
    nrm, _, _, buf = _assert_normals(vm, N.default_params())
    dev = T._dev(B)
    ctx.profile_select("voxel_align_plane")
    out, res = _assert_plane_loop(vm, nrm, buf.data_ptr() + 16, B, dev, START(vs), A.default_params(vs), vs)
    assert ctx.profile_read()[1] == 2 * res["iterations"]  # the loop's launches, and the sums asked for again pose by pose
    ctx.profile_select(None)
    want_out, want_res, _ = restated_plane_loop(vs, lg)  # the CPU test's run: no slot placement matters
    assert TA._bits(out) == TA._bits(want_out) and res == want_res
    out1, res1 = _assert_plane_loop(vm, nrm, buf.data_ptr() + 16, B, dev, START(vs), A.default_params(vs, max_iters=1), vs, "MAX_ITERS")
    assert res1["iterations"] == 1 and TA._bits(out1) != TA._bits(START(vs))
    vm.close()


@pytest.mark.gpu
def test_the_plane_loop_ends_with_too_few_and_degenerate(ctx):
    vs = 0.1
    B = corner(11)
    vm = TA._build(ctx, [("insert", corner(10), TA._m(TRUTH))], vs, 0.0, 14)
    nrm, _, _, buf = _assert_normals(vm, N.default_params())
    dev = T._dev(B)
    far = A.displaced(TRUTH, [500.0, 0.0, 0.0], [0.0, 0.0, 0.0])
    out, res = _assert_plane_loop(vm, nrm, buf.data_ptr() + 16, B, dev, far, A.default_params(vs), vs, "TOO_FEW")
    assert res["iterations"] == 1 and res["first_matched"] == 0 and TA._bits(out) == TA._bits(far)
    _assert_plane_loop(vm, nrm, buf.data_ptr() + 16, B[:0], dev, START(vs), A.default_params(vs), vs, "TOO_FEW")  # n == 0
    vm.close()
    # one plane: every normal is (0, 0, 1), three freedoms are not held and the first pivot is exactly 0
    p = one_plane()
    vm = TA._build(ctx, [("insert", p, T.IDENT)], VS, 0.0, LOG2)
    nrm, c, _, buf = _assert_normals(vm, N.default_params())
    assert c[:5] == [144, 140, 4, 0, 0] and set(N.by_key(TA._frozen(vm)[0], nrm).values()) == {(0, 0, ONE, 0), NONE_BITS}
    pose = [1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    out, res = _assert_plane_loop(vm, nrm, buf.data_ptr() + 16, p, T._dev(p), pose, A.default_params(VS, min_matches=6), VS, "DEGENERATE")
    assert res["first_matched"] == 140 and res["iterations"] == 1 and TA._bits(out) == TA._bits(pose)
    vm.close()


@pytest.mark.gpu
def test_bad_arguments_launch_nothing_and_leave_the_map_usable(ctx):
    import torch
    from stereo_vo_amd import api
    L = ctx.L
    vs = 0.1
    B = corner(11)
    vm = TA._build(ctx, [("insert", corner(10), TA._m(TRUTH))], vs, 0.0, 14)
    nrm, _, d, good = _assert_normals(vm, N.default_params())
    nptr = good.data_ptr() + 16
    nb = torch.full(((vm.capacity + 2) * 4,), SENT32, dtype=torch.int32, device="cuda")
    cn = torch.full((N.N_COUNTS + 2,), SENT, dtype=torch.int64, device="cuda")
    t, c = T._dev(B), torch.full((N.PLANE_WORDS + 2,), SENT, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    mp = np.ascontiguousarray(TA._m(TRUTH)).ctypes.data_as(C.c_void_p)
    q = (C.c_double * 7)(*TRUTH)
    out = (C.c_double * 7)(*([7.0] * 7))
    res = api.VoxelAlignResult()
    res.status, res.iterations = 77, 77
    ok, nok = api.voxel_align_default_params(vs), api.voxel_normals_default_params()

    def NP(**kw):
        return C.byref(api._params(api.voxel_normals_default_params, None, **kw))

    def AP(**kw):
        return C.byref(api._params(lambda: api.voxel_align_default_params(vs), None, **kw))

    nrm_call = lambda prm=C.byref(nok), n=None, k=None: L.svo_voxel_map_normals_dev(
        vm.h, prm, nb.data_ptr() + 16 if n is None else n, cn.data_ptr() + 8 if k is None else k)
    sums = lambda nr=nptr, n=5, pts=None, mat=mp, prm=C.byref(ok), s=None: L.svo_voxel_map_align_plane_sums_dev(
        vm.h, nr, t.data_ptr() if pts is None else pts, n, mat, prm, c.data_ptr() + 8 if s is None else s)
    loop = lambda nr=nptr, n=5, pts=None, qi=q, prm=C.byref(ok), o=out, r=C.byref(res): L.svo_voxel_map_align_plane(
        vm.h, nr, t.data_ptr() if pts is None else pts, n, qi, prm, o, r)
    calls = [(lambda: nrm_call(prm=None), "null params"), (lambda: nrm_call(prm=NP(min_count=0)), "min_count"),
             (lambda: nrm_call(prm=NP(min_neighbours=2)), "min_neighbours"), (lambda: nrm_call(prm=NP(min_neighbours=28)), "min_neighbours"),
             (lambda: nrm_call(prm=NP(max_curvature=0.0)), "max_curvature"), (lambda: nrm_call(prm=NP(max_curvature=1.5)), "max_curvature"),
             (lambda: nrm_call(prm=NP(max_curvature=float("nan"))), "max_curvature"), (lambda: nrm_call(prm=NP(max_curvature=float("inf"))), "max_curvature"),
             (lambda: nrm_call(n=0), "null normals"), (lambda: nrm_call(n=nb.data_ptr() + 24), "16-byte"), (lambda: nrm_call(k=cn.data_ptr() + 12), "8-byte"),
             (lambda: nrm_call(prm=NP(min_count=0), n=0), "min_count"),  # the order
             (lambda: L.svo_voxel_map_normals(vm.h, C.byref(nok), None, None), "null normals"),
             (lambda: sums(nr=0, n=-1), "null normals"), (lambda: sums(nr=nptr + 8, n=-1), "16-byte"), (lambda: sums(n=-1), "n must not"),
             (lambda: sums(n=(1 << 20) + 1), "2^20"), (lambda: sums(mat=None), "c2w12"), (lambda: sums(prm=None), "params"),
             (lambda: sums(prm=AP(reach=2)), "reach"), (lambda: sums(prm=AP(max_dist=0.0)), "max_dist"), (lambda: sums(s=0), "sums"),
             (lambda: sums(s=c.data_ptr() + 12), "8-byte"), (lambda: sums(pts=0), "points"), (lambda: sums(pts=t.data_ptr() + 2), "4-byte"),
             (lambda: L.svo_voxel_map_align_plane_sums_pose7_dev(vm.h, 0, t.data_ptr(), -1, None, C.byref(ok), c.data_ptr() + 8), "null normals"),
             (lambda: L.svo_voxel_map_align_plane_sums_pose7_dev(vm.h, nptr, t.data_ptr(), -1, None, C.byref(ok), c.data_ptr() + 8), "n must not"),
             (lambda: L.svo_voxel_map_align_plane_sums_pose7_dev(vm.h, nptr, t.data_ptr(), 5, None, C.byref(ok), c.data_ptr() + 8), "pose7"),
             (lambda: loop(nr=0, n=-1), "null normals"), (lambda: loop(nr=nptr + 4), "16-byte"), (lambda: loop(n=-1), "n must not"),
             (lambda: loop(qi=None), "pose7_in"), (lambda: loop(o=None), "pose7_out"), (lambda: loop(r=None), "result"), (lambda: loop(prm=None), "params"),
             (lambda: loop(prm=AP(max_iters=0)), "max_iters"), (lambda: loop(pts=0), "points"), (lambda: loop(pts=t.data_ptr() + 1), "4-byte")]
    before, stats = TA._frozen(vm)
    for tag in ("voxel_normals", "voxel_align_plane"):
        ctx.profile_select(tag)
        for call, word in calls:
            assert call() == -1 and word in L.svo_last_error(ctx.h).decode(), (word, L.svo_last_error(ctx.h).decode())
        assert ctx.profile_read()[1] == 0
        ctx.profile_select(None)
    ctx.sync()
    assert (nb.cpu().numpy().view(np.uint32) == SENT32).all() and cn.cpu().tolist() == [SENT] * (N.N_COUNTS + 2)
    assert c.cpu().tolist() == [SENT] * (N.PLANE_WORDS + 2) and list(out) == [7.0] * 7 and (res.status, res.iterations) == (77, 77)
    after, stats2 = TA._frozen(vm)
    assert all(np.array_equal(before[k], after[k]) for k in before) and stats2 == stats
    with pytest.raises(ValueError):
        vm.align_plane_sums(nptr, t.data_ptr(), 5, sums_ptr=c.data_ptr() + 8)
    # the context and the map work
    prm = A.default_params(vs)
    assert _plane_call(vm, nptr, B, prm, pose7=np.array(TRUTH)) == N.plane_sums_np(d, nrm, B, TA._m(TRUTH), vs, 0.0, prm)
    vm.close()
