"""The voxel map locate (include/svo.h, "Voxel map locate"): the occupancy volume, the scores and the host loop.

Without a GPU: the two routes of the restatement (tests/voxel_locate_ref.py) agree on every scene, every misreading changes a stated
scene, the corner scene is located from 0.7 to 1.7 m and 0.1 rad away at three voxel sizes, the two statuses that need no
refinement, the pure entries and the header under ASan + UBSan.  On the GPU: every word of the volume, the counts, the scores and
the bests with == into sentinel-filled guarded buffers, the loop's poses and result by bit pattern, and the table's bytes and the
map's counters before and after every call."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import voxel_align_ref as A
import voxel_locate_ref as L
import voxel_normals_ref as N
import voxel_ref as V
import test_voxel_align as TA
import test_voxel_map as T
import test_voxel_normals as TN
from test_host_sanitizers import _run_sanitized

TRUTH, VS, SENT = TA.TRUTH, TA.VS, TA.SENT
SENT32 = 0x5A5A5A5A
F32 = np.float32
# voxel size, table log2, box, the start's shift (m) and turn about the world's y (rad): the issue's table
CORNER = ((0.1, 14, (8, 4, 8), (0.53, -0.17, 0.42), 0.11), (0.05, 14, (16, 4, 16), (0.53, -0.12, -0.42), 0.11),
          (0.25, 12, (8, 4, 8), (1.3, -0.4, 1.1), -0.09))
# what the restatement gives: the peak's k, shift and hits, the next candidate's hits_max, the chosen rank (plane, point)
CORNER_WANT = {0.1: (7, (-6, 2, -4), 10266, 9535, (0, 0)), 0.05: (7, (-11, 2, 9), 7906, 6941, (2, 0)), 0.25: (3, (-6, 2, -4), 10743, 10559, (0, 0))}
ORIGIN, DIMS = (-20, -1, 7), (128, 4, 4)  # the constructed scenes' volume at VS: cell j is voxel ORIGIN + j
CHUNK = 1024  # records per workgroup of the score launch; test_pure_entries holds it to the library's


# ----------------------------------------------------------------------------------------------------- scenes without a GPU
def at(j, frac=(0.5, 0.5, 0.5)):
    """One record in cell j of the constructed volume."""
    return TA.rec(tuple(ORIGIN[r] + j[r] for r in range(3)), frac)


@functools.lru_cache(maxsize=None)
def random_words():
    rng = np.random.default_rng(20)
    w = rng.integers(0, 1 << 63, L.occupancy_words(DIMS), dtype=np.uint64) ^ (rng.integers(0, 2, L.occupancy_words(DIMS), dtype=np.uint64) << np.uint64(63))
    w.setflags(write=False)
    return w


def full_words():
    return np.full(L.occupancy_words(DIMS), ~np.uint64(0), np.uint64)


@functools.lru_cache(maxsize=None)
def random_records(n, seed=21):
    """n records in and around the constructed volume (up to three cells outside on every side)."""
    rng = np.random.default_rng(seed)
    cells = np.stack([rng.integers(-3, DIMS[r] + 3, n) for r in range(3)], axis=1)
    return TA.cat(*[at(tuple(int(v) for v in c)) for c in cells])


@functools.lru_cache(maxsize=None)
def score_scenes():
    """name -> (words, records, matrices, box): the constructed scenes of the scores at VS in the (128, 4, 4) volume.  `small`
    scenes also go through the Python route."""
    out = {}
    I = TA.ident()
    rw, fw = random_words(), full_words()
    for r0 in (16, 1, 0):
        # a window that starts at bit 0 of a word, one that ends at bit 63, one that straddles 63 | 64 (r0 = 0: the bits 63 and 64)
        pts = TA.cat(at((64 + r0, 1, 1)), at((63 - r0, 2, 2)), at((63, 1, 2)), at((64, 2, 1)))
        out[f"windows_r{r0}"] = (rw, pts, I, (r0, 1, 1))
        # the ends of the rows, of the axes and of the volume, every bit set: a bit of the next row would count
        ends = TA.cat(*[at(j) for j in ((0, 1, 1), (127, 1, 1), (0, 0, 0), (127, 3, 3), (5, 0, 2), (5, 3, 2), (5, 2, 0), (5, 2, 3), (127, 3, 0), (0, 0, 3))])
        out[f"row_ends_r{r0}"] = (fw, ends, I, (r0, 1, 1))
        out[f"row_ends_random_r{r0}"] = (rw, ends, I, (r0, 1, 1))
    out["box_0"] = (rw, random_records(40), I, (0, 0, 0))
    out["box_16"] = (rw, random_records(40), I, (16, 16, 16))
    out["box_16_full"] = (fw, random_records(12, 22), I, (16, 16, 16))
    for n in (1, 63, 64, 65, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1):
        out[f"n_{n}"] = (rw, random_records(CHUNK + 1)[:n], I, (2, 1, 1))
    # the flush of the planes.  A box of 64 rows or more gives an item a quarter of a chunk, 256 identical records that all hit: every
    # flush window of 63 records fills its counters to the top and an item flushes five times.  With fewer rows (the 64-part
    # path) an item walks 16 records.  The third box has rows whose every shift hits and rows none of whose does.
    for n in (4100, 70000):
        out[f"depth_{n}"] = (rw, np.repeat(at((70, 2, 1)), n), I, (16, 4, 4))
        out[f"depth_{n}_full"] = (fw, np.repeat(at((70, 2, 1)), n), I, (16, 16, 16))
        out[f"depth_{n}_few_rows"] = (rw, np.repeat(at((70, 2, 1)), n), I, (16, 1, 1))
    out["K_63"] = (rw, random_records(50), np.stack([TA.ident((0.25 * (k % 9 - 4), 0.25 * (k % 3 - 1), 0.25 * (k // 21 - 1))) for k in range(63)]), (1, 1, 1))
    out["K_33"] = (rw, random_records(50), np.stack([TA.ident((0.25 * (k % 7 - 3), 0.0, 0.0)) for k in range(33)]), (2, 0, 1))
    # two equal peaks in one candidate: the smallest index wins
    two = L.bits_of([(10, 1, 1), (12, 1, 1)], DIMS)
    out["tie"] = (two, at((11, 1, 1)), I, (2, 1, 1))
    out["all_zero"] = (np.zeros(L.occupancy_words(DIMS), np.uint64), random_records(40), I, (1, 1, 1))
    # rejected records: a NaN, z <= 0, |x| = 1024, and q_r at both ends of rule 1 (x = 0.5, shifted by the matrix)
    f = lambda x, y, z: V.records([F32(x)], [F32(y)], [F32(z)], np.array([0], np.uint32))
    below = np.nextafter(F32(1024), F32(0))
    odd = TA.cat(f(np.nan, 1, 2), f(1, 1, np.nan), f(1, 1, 0), f(1, 1, -2), f(1024, 0, 2), f(-1024, 0, 2), f(0, 1024, 2), f(below, 0.1, 2), f(0.1, -below, 2), at((3, 1, 1)))
    out["rejected"] = (rw, odd, I, (1, 1, 1))
    lo, hi = -262140.5, 262139.5
    ends = np.stack([TA.ident((float(t), 0.0, 0.0)) for t in (lo, np.nextafter(lo, -np.inf), hi, np.nextafter(hi, 0.0))])
    out["q_ends"] = (rw, TA.cat(TA.rec((2, 0, 8), (0.0, 0.5, 0.5)), at((3, 1, 1))), ends, (1, 1, 1))
    return out


SMALL = lambda name, n: n <= 300 and not name.startswith("box_16")  # what the Python route can afford


def want_scores(name):
    w, pts, mats, box = score_scenes()[name]
    return L.scores_np(w, ORIGIN, DIMS, pts, mats, box, VS, 0.0)


@functools.lru_cache(maxsize=None)
def occupancy_scenes():
    """name -> (steps of a 2^8 table at VS, origin, dims, min_count)."""
    O = (-3, -2, 5)
    out = {}
    for dims in ((64, 1, 1), (64, 8, 8)):
        d = dims
        faces = [(0, 0, 0), (d[0] - 1, 0, 0), (0, d[1] - 1, 0), (0, 0, d[2] - 1), (d[0] - 1, d[1] - 1, d[2] - 1), (31, d[1] // 2, d[2] // 2)]
        outside = [(-1, 0, 0), (d[0], 0, 0), (0, d[1], 0), (0, -1, 0), (0, 0, d[2]), (0, 0, -1)]
        cells = [tuple(O[r] + j[r] for r in range(3)) for j in faces + outside]
        cells = [c for c in cells if c[2] >= 1]
        steps = [("insert", TA.cat(*[TA.rec(c) for c in cells]), TA.ident())]
        out[f"faces_{d[1]}"] = (steps, O, dims, 1)
        twice = steps + [("insert", TA.cat(TA.rec(cells[0]), TA.rec(cells[0]), TA.rec(cells[1])), TA.ident())]
        out[f"min_count_3_{d[1]}"] = (twice, O, dims, 3)
        carved = steps + [("remove", TA.rec(cells[1]), TA.ident())]  # a removal's emptied voxel is exactly a carved one
        out[f"carved_{d[1]}"] = (carved, O, dims, 1)
    # both ends of the key range: a record moved there by the matrix, a volume that ends where the key range does
    lo, hi = -(1 << 20), (1 << 20) - 1
    far = [("insert", TA.rec((2, 2, 8)), TA.ident(((lo - 2) * VS, 0.0, 0.0))), ("insert", TA.rec((2, 2, 8)), TA.ident(((hi - 2) * VS, 0.0, 0.0)))]
    out["key_range_low"] = (far, (lo, 2, 8), (64, 1, 1), 1)
    out["key_range_high"] = (far, (hi - 63, 2, 8), (64, 1, 1), 1)
    return out


def test_the_two_routes_of_the_restatement_agree_on_every_scene():
    for name, (w, pts, mats, box) in score_scenes().items():
        hits, best = want_scores(name)
        K = len(np.asarray(mats).reshape(-1, 12))
        assert hits.shape == (K, (2 * box[0] + 1) * (2 * box[1] + 1) * (2 * box[2] + 1)) and int(hits.max()) == int(best["hits_max"].max())
        if SMALL(name, len(pts) * K):
            hp, bp = L.scores_py(L.live_of_words(w, ORIGIN, DIMS), ORIGIN, DIMS, pts, mats, box, VS, 0.0)
            assert np.array_equal(hits, hp) and best.tobytes() == bp.tobytes(), name
    for name, (steps, origin, dims, mc) in occupancy_scenes().items():
        d = TA.cpu_table(steps, VS, 0.0, 8)
        (wa, ca), (wb, cb) = L.occupancy_np(d, origin, dims, mc), L.occupancy_py(d, origin, dims, mc)
        assert np.array_equal(wa, wb) and ca == cb, name
    # the corner scene, thinned: through the occupancy of its table, three candidates, a box of 75 shifts
    vs, lg = 0.1, 14
    d = TN.corner_table(vs, lg)
    prm = L.default_params(n_turn=1, box=(2, 1, 2), dims=(128, 64, 128))
    T0, _, mats = L.candidates(TA.START(vs), prm)
    origin = L.origin_of(T0, vs, prm.dims)
    (wa, ca), (wb, cb) = L.occupancy_np(d, origin, prm.dims, 1), L.occupancy_py(d, origin, prm.dims, 1)
    assert np.array_equal(wa, wb) and ca == cb and ca[0] > 1000
    hits, best = L.both(wa, origin, prm.dims, TN.corner(11)[::40], mats, prm.box, vs, 0.0)
    assert int(best["hits_max"].max()) > 100


def test_the_scenes_are_what_they_were_built_to_be():
    S = score_scenes()
    hits, best = want_scores("tie")
    assert hits[0].tolist().count(1) == 2 and hits[0].sum() == 2 and (best["s0"][0], best["s1"][0], best["s2"][0]) == (-1, 0, 0)
    hits, best = want_scores("all_zero")
    assert not hits.any() and best["index"][0] == 0 and (best["s0"][0], best["s1"][0], best["s2"][0]) == (-1, -1, -1) and best["n_used"][0] == 40
    hits, best = want_scores("rejected")
    assert best["n_used"][0] == 3 and best["n_inside"][0] == 1
    hits, best = want_scores("q_ends")
    assert best["n_used"].tolist() == [1, 0, 1, 2] and best["n_inside"].tolist() == [0, 0, 0, 0]  # the second record is rejected at the low end
    for n in (4100, 70000):
        for tail in ("", "_full", "_few_rows"):
            hits, best = want_scores(f"depth_{n}{tail}")
            assert set(hits[0].tolist()) <= {0, n} and best["hits_max"][0] == n
        hits, _ = want_scores(f"depth_{n}_full")  # every bit set: a hit for every shift that stays inside (4 x 4 rows of 33)
        assert (hits[0] == n).sum() == 33 * 4 * 4
        rows = want_scores(f"depth_{n}")[0][0].reshape(81, 33)
        assert (rows == n).any() and 5 < (rows == n).mean() * 100 < 95
    # every bit set: a record's score under shift s is 1 iff j + s is inside, so the scores count the cells inside
    hits, best = want_scores("row_ends_r16")
    pts = S["row_ends_r16"][1]
    assert hits[0].sum() == sum((min(127, j0 + 16) - max(0, j0 - 16) + 1) * (min(3, j1 + 1) - max(0, j1 - 1) + 1) * (min(3, j2 + 1) - max(0, j2 - 1) + 1)
                                for j0, j1, j2 in ((0, 1, 1), (127, 1, 1), (0, 0, 0), (127, 3, 3), (5, 0, 2), (5, 3, 2), (5, 2, 0), (5, 2, 3), (127, 3, 0), (0, 0, 3)))
    assert len(pts) == 10
    occ = occupancy_scenes()
    d = TA.cpu_table(occ["faces_8"][0], VS, 0.0, 8)
    assert L.occupancy_np(d, *occ["faces_8"][1:])[1] == [6, 6] and L.occupancy_np(TA.cpu_table(occ["carved_8"][0], VS, 0.0, 8), *occ["carved_8"][1:])[1] == [5, 6]
    assert L.occupancy_np(TA.cpu_table(occ["min_count_3_8"][0], VS, 0.0, 8), *occ["min_count_3_8"][1:])[1] == [1, 0]
    for name in ("key_range_low", "key_range_high"):
        w, c = L.occupancy_np(TA.cpu_table(occ[name][0], VS, 0.0, 8), *occ[name][1:])
        assert c == [1, 1] and int(w[0]) == (1 if name.endswith("low") else 1 << 63)


def test_every_misreading_of_the_contract_changes_a_stated_scene():
    w, pts, mats, box = score_scenes()["tie"]
    base = L.scores_np(w, ORIGIN, DIMS, pts, mats, box, VS, 0.0)
    assert L.scores_np(w, ORIGIN, DIMS, pts, mats, box, VS, 0.0, variant="tie_largest")[1].tobytes() != base[1].tobytes()
    w, pts, mats, box = score_scenes()["windows_r1"]
    base = L.scores_np(w, ORIGIN, DIMS, pts, mats, box, VS, 0.0)
    for v in ("j_minus_s", "axis_order"):
        assert not np.array_equal(L.scores_np(w, ORIGIN, DIMS, pts, mats, box, VS, 0.0, variant=v)[0], base[0]), v
    w, pts, mats, box = score_scenes()["row_ends_r1"]
    assert not np.array_equal(L.scores_np(w, ORIGIN, DIMS, pts, mats, box, VS, 0.0, variant="outside_hits")[0], L.scores_np(w, ORIGIN, DIMS, pts, mats, box, VS, 0.0)[0])
    occ = occupancy_scenes()
    d = TA.cpu_table(occ["min_count_3_8"][0], VS, 0.0, 8)
    assert L.occupancy_np(d, *occ["min_count_3_8"][1:], variant="count_gt")[1] != L.occupancy_np(d, *occ["min_count_3_8"][1:])[1]
    d = TA.cpu_table(occ["faces_8"][0], VS, 0.0, 8)
    assert not np.array_equal(L.occupancy_np(d, *occ["faces_8"][1:], variant="bit_63")[0], L.occupancy_np(d, *occ["faces_8"][1:])[0])
    # the turn on the camera side is a turn about the camera's y, not the world's: with the camera pitched, another matrix
    prm, pitched = L.default_params(), [0.8, 0.3, -0.4, 0.2, 1.0, 2.0, 3.0]
    assert L.candidates(pitched, prm, variant="camera_side")[2][0] != L.candidates(pitched, prm)[2][0]
    assert L.candidates(pitched, prm, variant="camera_side")[2][prm.n_turn] == L.candidates(pitched, prm)[2][prm.n_turn]  # b = 0: no turn
    assert len(L.VARIANTS) == 7


def test_candidates_turn_about_the_world_axis_by_two_atan_b():
    prm = L.default_params(n_turn=31, turn_step=0.25)
    T0, us, mats = L.candidates(TRUTH, prm)
    u, T1 = A.from_pose7(TRUTH)
    R0 = np.array(A.quat_to_R(u)).reshape(3, 3)
    assert T0 == T1
    for k, uk in enumerate(us):
        b = (k - 31) * 0.25 / 2.0
        ang = 2.0 * math.atan(b)
        Ry = np.array([[math.cos(ang), 0.0, math.sin(ang)], [0.0, 1.0, 0.0], [-math.sin(ang), 0.0, math.cos(ang)]])
        assert np.allclose(np.array(A.quat_to_R(uk)).reshape(3, 3), Ry @ R0, rtol=0, atol=1e-14), k
        assert abs(math.sqrt(sum(v * v for v in uk)) - 1.0) <= 2.3e-16, k


# ----------------------------------------------------------------------------------------------------- the corner scene
def corner_start(vs):
    _, _, _, shift, ang = next(row for row in CORNER if row[0] == vs)
    return L.start_pose(TRUTH, shift, ang)


def restated(d, nrm, pts, start, prm, ap, vs, md=0.0):
    """The loop restated over a downloaded table (nrm None: the point form)."""
    def scores_at(origin, mats):
        w, _ = L.occupancy_np(d, origin, prm.dims, prm.min_count)
        return L.scores_np(w, origin, prm.dims, pts, mats, prm.box, vs, md)[1]

    def refine(pose):
        if nrm is None:
            out, res, _ = A.loop(pose, ap, lambda m: A.sums_np(d, pts, m, vs, md, ap))
        else:
            out, res, _ = N.plane_loop(pose, ap, lambda m: N.plane_sums_np(d, nrm, pts, m, vs, md, ap))
        return out, res
    return L.loop(start, prm, vs, scores_at, refine)


@functools.lru_cache(maxsize=None)
def restated_corner(vs, plane):
    _, lg, box, _, _ = next(row for row in CORNER if row[0] == vs)
    nrm = TN.corner_normals(vs, lg)[0] if plane else None
    return restated(TN.corner_table(vs, lg), nrm, TN.corner(11), corner_start(vs), L.default_params(box=box), A.default_params(vs), vs)


def test_the_corner_scene_is_located_from_several_voxels_away():
    """Seed 10 in the map under TRUTH, seed 11 located from TRUTH moved by `shift` and turned by `ang` about the world's y.  What
    the restatement gives (translation error in m / rotation error in rad; the start is 0.70 / 0.11, 0.69 / 0.11, 1.75 / 0.09):

      voxel   box        peak k  peak shift    hits    next candidate  peak's coarse pose  end, plane         end, point
      0.1 m   (8,4,8)    7       (-6, 2, -4)   10,266  9,535           0.0787 / 0.0099     0.0022 / 0.00077   0.0032 / 0.0026
      0.05 m  (16,4,16)  7       (-11, 2, 9)   7,906   6,941           0.0412 / 0.0099     0.0014 / 0.00052   0.0029 / 0.0013
      0.25 m  (8,4,8)    3       (-6, 2, -4)   10,743  10,559          0.2449 / 0.0500     0.0079 / 0.0028    0.0151 / 0.0104

    At 0.05 m the plane form's selection takes rank 2 (k = 8, shift (-13, 3, 9), 5,404 hits, 0.127 m from the truth before its
    refinement): its refinement matches more records than rank 0's.  The coarse bound below is therefore stated for the search
    peak, rank 0, whose coarse pose the trace holds; the chosen candidate's end is inside the bounds all the same."""
    for vs, lg, box, shift, ang in CORNER:
        for col, plane in enumerate((True, False)):
            out, res, (origin, mats, best, runs) = restated_corner(vs, plane)
            k, s, hits, nxt, ranks = CORNER_WANT[vs]
            top = L.rank(best, 64)
            (t0, r0), (tc, rc), (t1, r1) = A.pose_errors(corner_start(vs), TRUTH), A.pose_errors(runs[0][0], TRUTH), A.pose_errors(out, TRUTH)
            print(f"corner {vs} {'plane' if plane else 'point'}: start {t0:.4f} {r0:.4f}  peak {tc:.4f} {rc:.5f}  end {t1:.5f} {r1:.5f}  {res}")
            assert (top[0], (int(best['s0'][k]), int(best['s1'][k]), int(best['s2'][k])), int(best["hits_max"][k]), int(best["hits_max"][top[1]])) == (k, s, hits, nxt)
            assert res["status"] == "FOUND" and res["rank"] == ranks[col] and res["n_refined"] == 3
            assert t0 > 6 * vs and tc < 1.5 * vs and t1 < vs / 2 and r1 < 0.04 / 2 and t1 < tc and r1 < rc, (vs, plane, t0, tc, t1, rc, r1)


def test_an_empty_map_has_no_candidate_and_points_on_the_axis_stay_unrefined():
    vs = 0.1
    empty = TA.cpu_table([], vs, 0.0, 8)
    start = corner_start(vs)
    out, res, _ = restated(empty, None, TN.corner(11), start, L.default_params(), A.default_params(vs), vs)
    assert res["status"] == "NO_CANDIDATE" and TA._bits(out) == TA._bits(start) and (res["k"], res["rank"], res["n_refined"]) == (-1, -1, 0)
    line, pose, prm, ap = line_scene()
    d = TA.cpu_table([("insert", line, T.IDENT)], vs, 0.0, 8)
    out, res, (_, _, best, runs) = restated(d, None, line, pose, prm, ap, vs)
    assert res["status"] == "UNREFINED" and res["align"]["status"] == "DEGENERATE" and res["hits"] == 8 and res["shift"] == (0, 0, 0)
    assert TA._bits(out) == TA._bits(res["coarse_pose7"]) == TA._bits(runs[0][0]) and res["n_refined"] == 1


def line_scene():
    """Section 7q's DEGENERATE scene: eight points on the camera's axis, located in a map that holds them."""
    line = V.records(np.zeros(8, F32), np.zeros(8, F32), (1.0 + 0.37 * np.arange(8)).astype(F32), np.arange(8, dtype=np.uint32))
    return line, [1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], L.default_params(n_turn=1, box=(1, 1, 1), dims=(64, 64, 128), min_hits=8), A.default_params(0.1, min_matches=6)


def test_pure_entries_and_refusals_without_a_context():
    from stereo_vo_amd import api
    lib = api.lib()
    p = api.voxel_locate_default_params(0.1)
    want = L.default_params()
    assert (p.min_count, p.up_axis, p.n_turn, p.turn_step, tuple(p.box), tuple(p.dims), p.n_refine, p.min_hits) == tuple(want)
    assert C.sizeof(api.VoxelLocateParams) == 48 and C.sizeof(api.VoxelLocateResult) == 176 and api.VoxelLocateBest.itemsize == 32 and api.VoxelLocateBest == L.BEST
    assert api.VOXEL_LOCATE_STATUS == L.STATUS and api.VOXEL_LOCATE_CHUNK == CHUNK
    assert lib.svo_voxel_locate_default_params(C.c_float(0.1), None) == -1 and lib.svo_voxel_locate_default_params(C.c_float(0.0), C.byref(p)) == -1
    assert api.voxel_occupancy_bytes((512, 128, 512)) == 4 << 20 and api.voxel_occupancy_bytes((64, 1, 1)) == 8 and api.voxel_occupancy_bytes((1024, 1024, 1024)) == 1 << 27
    for bad in ((0, 1, 1), (32, 1, 1), (96, 1, 1), (64, 0, 1), (64, 1, 2049), (2112, 1, 1), (2048, 1024, 1024)):
        with pytest.raises(api.SvoError):
            api.voxel_occupancy_bytes(bad)
    assert api.voxel_locate_workspace_bytes(p) == L.workspace_bytes(want) == (4 << 20) + 256 + 93696 + 512
    for prm in (want._replace(n_turn=31, box=(16, 16, 16)), want._replace(n_turn=0, box=(0, 0, 0), dims=(64, 1, 1))):
        q = api._params(lambda: api.voxel_locate_default_params(0.1), None, n_turn=prm.n_turn)
        q.box, q.dims = (C.c_int * 3)(*prm.box), (C.c_int * 3)(*prm.dims)
        assert api.voxel_locate_workspace_bytes(q) == L.workspace_bytes(prm)
    for name, value in (("min_count", 0), ("up_axis", 3), ("up_axis", -1), ("n_turn", 32), ("n_turn", -1), ("turn_step", 0.0), ("turn_step", 0.26),
                        ("turn_step", float("nan")), ("n_refine", 0), ("n_refine", 64), ("min_hits", 0)):
        with pytest.raises(api.SvoError):
            api.voxel_locate_workspace_bytes(api._params(lambda: api.voxel_locate_default_params(0.1), None, **{name: value}))
    for field, value in (("box", (17, 0, 0)), ("box", (0, -1, 0)), ("dims", (100, 1, 1)), ("dims", (64, 1, 0))):
        q = api.voxel_locate_default_params(0.1)
        setattr(q, field, (C.c_int * 3)(*value))
        with pytest.raises(api.SvoError):
            api.voxel_locate_workspace_bytes(q)
    n = C.c_size_t(7)
    assert lib.svo_voxel_locate_workspace_bytes(None, C.byref(n)) == -1 and n.value == 0 and lib.svo_voxel_locate_workspace_bytes(C.byref(p), None) == -1
    buf, i3 = (C.c_double * 12)(), (C.c_int * 3)(64, 1, 1)
    ap, res = api.voxel_align_default_params(0.1), api.VoxelLocateResult()
    assert lib.svo_voxel_map_occupancy_dev(None, 1, i3, i3, buf, buf) == -1 and lib.svo_voxel_map_occupancy(None, 1, i3, i3, buf, buf) == -1
    assert lib.svo_voxel_map_locate_scores_dev(None, buf, i3, i3, None, 0, buf, 1, i3, buf, buf) == -1
    assert lib.svo_voxel_map_locate(None, None, None, 0, buf, C.byref(p), C.byref(ap), buf, buf, C.byref(res)) == -1


def test_voxel_locate_host_logic_under_sanitizers(tmp_path):
    """host/voxel_locate.h on the CPU under ASan + UBSan: every refusal at its boundary with code, message and order, the sizes, the
    candidates of 10,000 random poses (| |u_k| - 1 | within one ulp), the ranking and the selection on constructed bests, the
    loop's three statuses over stub functors, and the candidate matrices of the Python restatement bit for bit."""
    prm = L.default_params(n_turn=2, turn_step=0.25, up_axis=2)
    args = []
    for pose in (TRUTH, corner_start(0.1)):
        _, us, mats = L.candidates(pose, prm)
        args += [np.float64(v).view(np.uint64).item().__format__("x") for v in list(pose) + [x for m in mats for x in m]]
    _run_sanitized(tmp_path, "voxel_locate_args_test", "voxel locate args ok", *args)


# ===================================================================================================== GPU
def _guarded(words, dtype, sent):
    """A device buffer of `words` elements with one 256-byte guard of sentinels on each side: (tensor, pointer, guard elements)."""
    import torch
    g = 256 // torch.empty((), dtype=dtype).element_size()
    t = torch.full((words + 2 * g,), sent, dtype=dtype, device="cuda")
    return t, t.data_ptr() + 256, g


def _unguard(t, g, sent):
    a = t.cpu().numpy()
    assert (a[:g] == sent).all() and (a[-g:] == sent).all()
    return a[g:-g].copy()


def _occupancy_call(vm, origin, dims, mc):
    """One occupancy launch into guarded buffers: (the words, the two counts, the downloaded table, the volume's tensor and pointer)."""
    import torch
    before, stats = TA._frozen(vm)
    bt, bp, bg = _guarded(L.occupancy_words(dims), torch.int64, SENT)
    ct, cp, cg = _guarded(2, torch.int32, SENT32)
    torch.cuda.synchronize()
    vm.occupancy(bp, origin, dims, min_count=mc, counts_ptr=cp)
    vm.ctx.sync()
    words, counts = _unguard(bt, bg, SENT).view(np.uint64), _unguard(ct, cg, SENT32).view(np.uint32).tolist()
    after, stats2 = TA._frozen(vm)
    assert all(np.array_equal(before[k], after[k]) for k in before) and stats2 == stats
    return words, counts, before, bt, bp


def _upload(words):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(words).view(np.int64).copy()).cuda()
    return t, t.data_ptr()


def _scores_call(vm, bits_ptr, origin, dims, pts, mats, box, dev=None):
    """One scores call into guarded buffers: (hits (K, S0 S1 S2) uint32, K BEST records)."""
    import torch
    before, stats = TA._frozen(vm)
    K = len(np.asarray(mats).reshape(-1, 12))
    SS = (2 * box[0] + 1) * (2 * box[1] + 1) * (2 * box[2] + 1)
    ht, hp, hg = _guarded(K * SS, torch.int32, SENT32)
    bt, bp, bg = _guarded(K * 8, torch.int32, SENT32)
    t = T._dev(pts) if dev is None and len(pts) else dev
    torch.cuda.synchronize()
    vm.locate_scores(bits_ptr, origin, dims, t.data_ptr() if len(pts) else None, len(pts), mats, box, hits_ptr=hp, best_ptr=bp)
    vm.ctx.sync()
    hits, best = _unguard(ht, hg, SENT32).view(np.uint32).reshape(K, SS), _unguard(bt, bg, SENT32).view(L.BEST)
    after, stats2 = TA._frozen(vm)
    assert all(np.array_equal(before[k], after[k]) for k in before) and stats2 == stats
    return hits, best


def _assert_scores(got, want, what):
    bad = np.argwhere(got[0] != want[0])
    assert len(bad) == 0, (what, bad[:8].tolist(), got[0][tuple(bad[0])], want[0][tuple(bad[0])])
    assert got[1].tobytes() == want[1].tobytes(), (what, got[1], want[1])


@pytest.mark.gpu
@pytest.mark.parametrize("vs,lg", TA.SIZES)
def test_corner_scene_occupancy(ctx, vs, lg):
    vm = TA._build(ctx, [("insert", TN.corner(10), TA._m(TRUTH))], vs, 0.0, lg)
    T0, _, _ = L.candidates(TRUTH, L.default_params())
    for dims in ((512, 128, 512), (64, 32, 128)):
        origin = L.origin_of(T0, vs, dims)
        for mc in (1, 3):
            words, counts, d, _, _ = _occupancy_call(vm, origin, dims, mc)
            want, wc = L.occupancy_np(d, origin, dims, mc)
            assert np.array_equal(words, want) and counts == wc, (vs, dims, mc)
            assert wc == L.occupancy_np(TN.corner_table(vs, lg), origin, dims, mc)[1] and wc[0] > 50  # no slot placement matters
    hw, hc = vm.occupancy_host(origin, dims, min_count=3)
    assert np.array_equal(hw, want) and [hc["n_inside"], hc["n_outside"]] == wc
    vm.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(occupancy_scenes()))
def test_constructed_occupancy(ctx, name):
    steps, origin, dims, mc = occupancy_scenes()[name]
    vm = TA._build(ctx, steps, VS, 0.0, 8)
    words, counts, d, _, _ = _occupancy_call(vm, origin, dims, mc)
    want, wc = L.occupancy_py(d, origin, dims, mc)
    assert np.array_equal(words, want) and counts == wc
    assert wc == L.occupancy_np(TA.cpu_table(steps, VS, 0.0, 8), origin, dims, mc)[1]
    vm.close()


@pytest.mark.gpu
def test_occupancy_of_a_full_table_and_the_profile_bracket(ctx):
    p, _ = TA.full_table()
    vm = TA._build(ctx, [("insert", p, T.IDENT)], 0.1, 0.0, 8)
    ctx.profile_select("voxel_occupancy")
    words, counts, d, _, _ = _occupancy_call(vm, (-32, -8, 8), (64, 16, 16), 1)
    assert ctx.profile_read()[1] == 1
    ctx.profile_select(None)
    want, wc = L.occupancy_py(d, (-32, -8, 8), (64, 16, 16), 1)
    assert (d["keys"] != np.uint64(V.EMPTY)).all() and np.array_equal(words, want) and counts == wc and sum(wc) == 256 and wc[0] > 20
    vm.close()


@pytest.mark.gpu
def test_constructed_scores(ctx):
    vm = T._map(ctx, VS, 8)
    ctx.profile_select("voxel_locate")
    calls = 0
    for name, (w, pts, mats, box) in score_scenes().items():
        t, ptr = _upload(w)
        _assert_scores(_scores_call(vm, ptr, ORIGIN, DIMS, pts, mats, box), want_scores(name), name)
        calls += 1
    # a repeated call into the same buffers gives the same words; n == 0 zeroes the scores and writes the all-zero bests
    w, pts, mats, box = score_scenes()["n_257"]
    t, ptr = _upload(w)
    dev = T._dev(pts)
    _assert_scores(_scores_call(vm, ptr, ORIGIN, DIMS, pts, mats, box, dev=dev), want_scores("n_257"), "again")
    hits, best = _scores_call(vm, ptr, ORIGIN, DIMS, pts[:0], mats, box)
    assert not hits.any() and best.tolist() == [(0, -2, -1, -1, 0, 0, 0, 0)]
    assert ctx.profile_read()[1] == calls + 2
    ctx.profile_select(None)
    vm.close()


@pytest.mark.gpu
def test_two_equal_peaks_in_both_table_orders(ctx):
    cells = [tuple(ORIGIN[r] + j[r] for r in range(3)) for j in ((10, 1, 1), (12, 1, 1))]
    for order in (cells, cells[::-1]):
        vm = TA._build(ctx, [("insert", TA.rec(c), TA.ident()) for c in order], VS, 0.0, 8)
        words, counts, _, _, ptr = _occupancy_call(vm, ORIGIN, DIMS, 1)
        assert counts == [2, 0] and np.array_equal(words, score_scenes()["tie"][0])
        _assert_scores(_scores_call(vm, ptr, ORIGIN, DIMS, at((11, 1, 1)), TA.ident(), (2, 1, 1)), want_scores("tie"), "tie")
        vm.close()


@pytest.mark.gpu
@pytest.mark.parametrize("vs,lg,box,shift,ang", CORNER)
def test_corner_scene_scores(ctx, vs, lg, box, shift, ang):
    vm = TA._build(ctx, [("insert", TN.corner(10), TA._m(TRUTH))], vs, 0.0, lg)
    prm = L.default_params(box=box)
    _, _, (origin, mats, best, _) = restated_corner(vs, False)
    words, counts, d, _, ptr = _occupancy_call(vm, origin, prm.dims, 1)
    want = L.scores_np(L.occupancy_np(d, origin, prm.dims, 1)[0], origin, prm.dims, TN.corner(11), mats, box, vs, 0.0)
    assert want[1].tobytes() == best.tobytes()  # the CPU test's run: no slot placement matters
    _assert_scores(_scores_call(vm, ptr, origin, prm.dims, TN.corner(11), np.array(mats), box), want, vs)
    vm.close()


def _workspace(prm):
    import torch
    from stereo_vo_amd import api
    q = api._params(lambda: api.voxel_locate_default_params(0.1), None, **{k: v for k, v in prm._asdict().items() if k not in ("box", "dims")})
    q.box, q.dims = (C.c_int * 3)(*prm.box), (C.c_int * 3)(*prm.dims)
    t = torch.empty(api.voxel_locate_workspace_bytes(q) + 256, dtype=torch.uint8, device="cuda")
    return t, (t.data_ptr() + 255) & ~255, q


def _assert_locate(vm, nrm, nptr, pts, dev, start, prm, ap, vs, want_status=None):
    """svo_voxel_map_locate against the restatement's loop over the downloaded table: pose7_out, coarse_pose7 and xi by bit pattern
    and every field of the result."""
    before, stats = TA._frozen(vm)
    out, res, trace = restated(before, nrm, pts, start, prm, ap, vs)
    ws, wptr, q = _workspace(prm)
    got_out, got = vm.locate(dev.data_ptr() if len(pts) else None, len(pts), np.array(start), params=q, align_params=_align_params(ap, vs), normals_ptr=nptr,
                             workspace_ptr=wptr)
    assert TA._bits(got_out) == TA._bits(out), (got_out, out, got, res)
    assert TA._bits(got["coarse_pose7"]) == TA._bits(res["coarse_pose7"]) and TA._bits(got["align"]["xi"]) == TA._bits(res["align"]["xi"])
    plain = lambda r: ({k: v for k, v in r.items() if k not in ("coarse_pose7", "align")}, {k: v for k, v in r["align"].items() if k != "xi"})
    assert plain(got) == plain(res), (got, res)
    after, stats2 = TA._frozen(vm)
    assert all(np.array_equal(before[k], after[k]) for k in before) and stats2 == stats
    if want_status is not None:
        assert res["status"] == want_status, res
    return out, res


def _align_params(ap, vs):
    from stereo_vo_amd import api
    return api._params(lambda: api.voxel_align_default_params(vs), None, **ap._asdict())


@pytest.mark.gpu
@pytest.mark.parametrize("vs,lg,box,shift,ang", CORNER)
def test_the_loop_equals_the_restatement_in_every_bit(ctx, vs, lg, box, shift, ang):
    B = TN.corner(11)
    vm = TA._build(ctx, [("insert", TN.corner(10), TA._m(TRUTH))], vs, 0.0, lg)
    nrm, _, _, buf = TN._assert_normals(vm, N.default_params())
    dev = T._dev(B)
    prm, ap = L.default_params(box=box), A.default_params(vs)
    for plane in (True, False):
        ctx.profile_select("voxel_locate")
        out, res = _assert_locate(vm, nrm if plane else None, buf.data_ptr() + 16 if plane else None, B, dev, corner_start(vs), prm, ap, vs, "FOUND")
        assert ctx.profile_read()[1] == 1
        ctx.profile_select(None)
        want_out, want_res, _ = restated_corner(vs, plane)  # the CPU test's run
        assert TA._bits(out) == TA._bits(want_out) and res == want_res
    vm.close()


@pytest.mark.gpu
def test_the_loop_ends_with_no_candidate_and_unrefined(ctx):
    vs = 0.1
    B = TN.corner(11)
    vm = T._map(ctx, vs, 8)
    out, res = _assert_locate(vm, None, None, B, T._dev(B), corner_start(vs), L.default_params(), A.default_params(vs), vs, "NO_CANDIDATE")
    assert TA._bits(out) == TA._bits(corner_start(vs))
    vm.close()
    line, pose, prm, ap = line_scene()
    vm = TA._build(ctx, [("insert", line, T.IDENT)], vs, 0.0, 8)
    _assert_locate(vm, None, None, line, T._dev(line), pose, prm, ap, vs, "UNREFINED")
    _assert_locate(vm, None, None, line[:0], None, pose, prm, ap, vs, "NO_CANDIDATE")  # n == 0
    vm.close()


@pytest.mark.gpu
def test_bad_arguments_launch_nothing_and_leave_the_map_usable(ctx):
    import torch
    from stereo_vo_amd import api
    lib = ctx.L
    vs = 0.1
    B = TN.corner(11)
    vm = TA._build(ctx, [("insert", TN.corner(10), TA._m(TRUTH))], vs, 0.0, 14)
    dims, box = (64, 8, 8), (1, 1, 1)
    bt, bp, bg = _guarded(L.occupancy_words(dims), torch.int64, SENT)
    ct, cp, cg = _guarded(2, torch.int32, SENT32)
    ht, hp, hg = _guarded(27, torch.int32, SENT32)
    et, ep, eg = _guarded(8, torch.int32, SENT32)
    ws, wptr, ok = _workspace(L.default_params(dims=dims, box=box))
    ws.fill_(0x5A)
    t = T._dev(B)
    torch.cuda.synchronize()
    I3 = lambda *v: (C.c_int * 3)(*v)
    o3, d3, b3 = I3(0, 0, 0), I3(*dims), I3(*box)
    mp = np.ascontiguousarray(TA._m(TRUTH)).ctypes.data_as(C.c_void_p)
    q = (C.c_double * 7)(*TRUTH)
    out = (C.c_double * 7)(*([7.0] * 7))
    res = api.VoxelLocateResult()
    res.status, res.k = 77, 77
    aok = api.voxel_align_default_params(vs)

    def LP(**kw):
        p = api.VoxelLocateParams.from_buffer_copy(ok)
        for k, v in kw.items():
            setattr(p, k, I3(*v) if k in ("box", "dims") else v)
        return C.byref(p)

    reach2 = api.VoxelAlignParams.from_buffer_copy(aok)
    reach2.reach = 2

    occ = lambda mc=1, o=o3, d=d3, b=None, c=None: lib.svo_voxel_map_occupancy_dev(vm.h, mc, o, d, bp if b is None else b, cp if c is None else c)
    sc = lambda b=None, o=o3, d=d3, pts=None, n=5, m=mp, K=1, bx=b3, h=None, e=None: lib.svo_voxel_map_locate_scores_dev(
        vm.h, bp if b is None else b, o, d, t.data_ptr() if pts is None else pts, n, m, K, bx, hp if h is None else h, ep if e is None else e)
    loc = lambda nr=None, pts=None, n=5, qi=q, p=C.byref(ok), a=C.byref(aok), w=None, o=out, r=C.byref(res): lib.svo_voxel_map_locate(
        vm.h, nr, t.data_ptr() if pts is None else pts, n, qi, p, a, wptr if w is None else w, o, r)
    calls = [(lambda: occ(mc=0), "min_count"), (lambda: occ(o=None), "null origin"), (lambda: occ(o=I3(-(1 << 20) - 1, 0, 0)), "origin outside"),
             (lambda: occ(o=I3(0, 1 << 20, 0)), "origin outside"), (lambda: occ(d=None), "null dims"), (lambda: occ(d=I3(64, 0, 1)), "dims outside"),
             (lambda: occ(d=I3(64, 1, 2049)), "dims outside"), (lambda: occ(d=I3(96, 1, 1)), "multiple of 64"), (lambda: occ(d=I3(2048, 1024, 1024)), "2^30"),
             (lambda: occ(b=0), "null bits"), (lambda: occ(b=bp + 4), "8-byte"), (lambda: occ(c=0), "null counts"), (lambda: occ(c=cp + 2), "4-byte"),
             (lambda: occ(mc=0, o=None), "min_count"),  # the order
             (lambda: lib.svo_voxel_map_occupancy(vm.h, 1, o3, d3, None, None), "null bits"),
             (lambda: sc(n=-1), "n must not"), (lambda: sc(n=(1 << 20) + 1), "2^20"), (lambda: sc(m=None), "null mats"), (lambda: sc(K=0), "K outside"),
             (lambda: sc(K=64), "K outside"), (lambda: sc(bx=None), "null box"), (lambda: sc(bx=I3(17, 0, 0)), "box outside"), (lambda: sc(bx=I3(0, 0, -1)), "box outside"),
             (lambda: sc(o=None), "null origin"), (lambda: sc(d=I3(32, 1, 1)), "multiple of 64"), (lambda: sc(b=0), "null bits"), (lambda: sc(b=bp + 4), "8-byte"),
             (lambda: sc(h=0), "null hits"), (lambda: sc(h=hp + 2), "4-byte"), (lambda: sc(e=0), "null best"), (lambda: sc(e=ep + 4), "8-byte"),
             (lambda: sc(pts=0), "null points"), (lambda: sc(pts=t.data_ptr() + 2), "4-byte"), (lambda: sc(n=-1, m=None), "n must not"),
             (lambda: loc(n=-1), "n must not"), (lambda: loc(n=(1 << 20) + 1), "2^20"), (lambda: loc(qi=None), "pose7_in"), (lambda: loc(o=None), "pose7_out"),
             (lambda: loc(r=None), "null result"), (lambda: loc(p=None), "null params"), (lambda: loc(p=LP(min_count=0)), "min_count"),
             (lambda: loc(p=LP(up_axis=3)), "up_axis"), (lambda: loc(p=LP(n_turn=32)), "n_turn"), (lambda: loc(p=LP(turn_step=0.3)), "turn_step"),
             (lambda: loc(p=LP(turn_step=float("nan"))), "turn_step"), (lambda: loc(p=LP(box=(0, 17, 0))), "box outside"), (lambda: loc(p=LP(dims=(64, 8, 0))), "dims outside"),
             (lambda: loc(p=LP(n_refine=0)), "n_refine"), (lambda: loc(p=LP(min_hits=0)), "min_hits"), (lambda: loc(a=None), "voxel_map_align: null params"),
             (lambda: loc(a=C.byref(reach2)), "reach"), (lambda: loc(w=0), "null workspace"), (lambda: loc(w=wptr + 128), "256-byte"),
             (lambda: loc(nr=bp + 8), "16-byte"), (lambda: loc(pts=0), "null points"), (lambda: loc(pts=t.data_ptr() + 1), "4-byte"),
             (lambda: loc(qi=(C.c_double * 7)(1.0, 0.0, 0.0, 0.0, 2.0e5, 0.0, 0.0)), "leaves the key range"),
             (lambda: loc(qi=(C.c_double * 7)(1.0, 0.0, 0.0, 0.0, float("nan"), 0.0, 0.0)), "outside the key range")]
    assert len(calls) >= 30
    before, stats = TA._frozen(vm)
    for tag in ("voxel_occupancy", "voxel_locate", "voxel_align"):
        ctx.profile_select(tag)
        for call, word in calls:
            assert call() == -1 and word in lib.svo_last_error(ctx.h).decode(), (word, lib.svo_last_error(ctx.h).decode())
        assert ctx.profile_read()[1] == 0
        ctx.profile_select(None)
    ctx.sync()
    for tt, g, s in ((bt, bg, SENT), (ct, cg, SENT32), (ht, hg, SENT32), (et, eg, SENT32)):
        assert (tt.cpu().numpy() == s).all()
    assert (ws.cpu().numpy() == 0x5A).all() and list(out) == [7.0] * 7 and (res.status, res.k) == (77, 77)
    after, stats2 = TA._frozen(vm)
    assert all(np.array_equal(before[k], after[k]) for k in before) and stats2 == stats
    # the context and the map work
    T0, _, _ = L.candidates(TRUTH, L.default_params())
    origin = L.origin_of(T0, vs, (64, 32, 128))
    words, counts, d, _, _ = _occupancy_call(vm, origin, (64, 32, 128), 1)
    assert np.array_equal(words, L.occupancy_np(d, origin, (64, 32, 128), 1)[0])
    vm.close()
