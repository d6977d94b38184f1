"""Voxel map distance field (include/svo.h, "Voxel map distance field"): the restatement's two routes against each other
and against scipy, the constructed scenes, the misreadings, the pure entries, the query's rule, the host logic under sanitizers, and
on the GPU every entry against the restatement with ==."""
import ctypes as C
import functools
import struct

import numpy as np
import pytest

import voxel_distance_ref as D
import test_voxel_align as TA
import test_voxel_map as T
import test_voxel_normals as TN
import test_voxel_rays as TR
from test_host_sanitizers import _run_sanitized
from test_voxel_locate import _guarded, _unguard, _occupancy_call

F32 = np.float32
VS = 0.5  # the constructed scenes: rule 4's pair 1.5 and the float below it are 3 voxels and just less
SENT, SENT32, SENT16 = TA.SENT, 0x5A5A5A5A, 0x5A5A
BELOW_1_5 = float(np.nextafter(F32(1.5), F32(0)))
ORIGIN = (-61, -3, -7)  # of the query's volume


def bits_of(cells, dims):
    occ = np.zeros((dims[2], dims[1], dims[0]), bool)
    for j0, j1, j2 in cells:
        occ[j2, j1, j0] = True
    return D.pack_bits(occ)


def random_words(dims, density, seed):
    rng = np.random.default_rng(seed)
    return D.pack_bits(rng.random((dims[2], dims[1], dims[0])) < density)


def corners(dims):
    return bits_of([(a, b, c) for a in (0, dims[0] - 1) for b in (0, dims[1] - 1) for c in (0, dims[2] - 1)], dims)


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> (dims, words, max_dist, inflate_radius).  Every shape, fill and max_dist of the issue's list, each where it can go wrong."""
    s = {}
    zero, ones = lambda d: np.zeros(d[0] * d[1] * d[2] // 64, np.uint64), lambda d: np.full(d[0] * d[1] * d[2] // 64, 2 ** 64 - 1, np.uint64)
    d = (64, 1, 1)
    s["64_zero"] = (d, zero(d), 5, 0.0)
    s["64_ones"] = (d, ones(d), 254, 1.5)
    s["64_ends_md1"] = (d, bits_of([(0, 0, 0), (63, 0, 0)], d), 1, 0.0)
    s["64_ends_md63"] = (d, bits_of([(0, 0, 0)], d), 63, 1.5)
    s["64_bit63_md64"] = (d, bits_of([(63, 0, 0)], d), 64, BELOW_1_5)
    s["64_random_md254"] = (d, random_words(d, 0.3, 1), 254, 1000.0)  # max_dist beyond every dim; R2 at the clamp
    d = (64, 3, 2)
    s["wrap"] = (d, bits_of([(63, 0, 0)], d), 3, 0.0)
    s["64x3x2_corners"] = (d, corners(d), 5, 1.5)
    d = (128, 9, 13)
    s["odd_0.01_md5"] = (d, random_words(d, 0.01, 2), 5, 1.5)
    s["odd_0.01_md5_below"] = (d, random_words(d, 0.01, 2), 5, BELOW_1_5)
    s["odd_0.3_md65"] = (d, random_words(d, 0.3, 3), 65, 0.0)
    s["odd_0.0005_md130"] = (d, random_words(d, 0.0005, 4), 130, 1000.0)
    s["odd_corners_md254"] = (d, corners(d), 254, 1.5)
    s["odd_words_md64"] = (d, bits_of([(0, 4, 6), (63, 0, 0), (64, 8, 12), (127, 4, 0)], d), 64, 1.5)
    s["odd_zero_md130"] = (d, zero(d), 130, 1.5)
    s["odd_ones_md5"] = (d, ones(d), 5, 0.0)
    d = (2048, 2, 2)
    for md in (63, 64, 65, 130, 254):  # the axis-0 pass crosses zero, one and several word boundaries and reaches the row's ends
        s[f"long_md{md}"] = (d, bits_of([(0, 0, 0), (63, 1, 0), (64, 0, 1), (127, 1, 1), (700, 0, 0), (1300, 1, 0), (2047, 1, 1)], d), md, 1.5)
    s["long_0.0005_md254"] = (d, random_words(d, 0.0005, 5), 254, 1000.0)
    s["long_corners_md130"] = (d, corners(d), 130, 0.0)
    d = (64, 2, 2048)
    s["deep_0.0005_md254"] = (d, random_words(d, 0.0005, 6), 254, 1.5)
    s["deep_0.01_md5"] = (d, random_words(d, 0.01, 7), 5, 1.5)
    d = (64, 2048, 2)
    s["tall_0.0005_md254"] = (d, random_words(d, 0.0005, 8), 254, 1.5)
    s["tall_corners_md130"] = (d, corners(d), 130, 1000.0)
    d = (192, 33, 31)
    s["mid_0.01_md63"] = (d, random_words(d, 0.01, 9), 63, 1.5)
    s["mid_0.0005_md130"] = (d, random_words(d, 0.0005, 10), 130, BELOW_1_5)
    d = (256, 64, 64)
    s["big_0.0005_md65"] = (d, random_words(d, 0.0005, 11), 65, 1.5)
    s["big_corners_md254"] = (d, corners(d), 254, 1000.0)
    s["big_0.3_md5"] = (d, random_words(d, 0.3, 12), 5, 0.0)
    return s


@functools.lru_cache(maxsize=None)
def want(name):
    dims, w, md, rad = scenes()[name]
    return D.field(w, dims, md, rad, VS)


def one_source():
    dims = (64, 16, 16)
    return dims, bits_of([(8, 8, 8)], dims), 7


def lattice():
    dims = (64, 8, 8)
    return dims, bits_of([(a, b, c) for a in range(0, 64, 4) for b in range(0, 8, 4) for c in range(0, 8, 4)], dims), 7


def test_the_two_routes_agree_and_match_scipy_on_every_scene():
    ndi = pytest.importorskip("scipy.ndimage")
    extra = {"one_source": one_source(), "lattice": lattice()}
    for name in list(scenes()) + list(extra):
        dims, w, md = (scenes()[name][:3]) if name in scenes() else extra[name]
        occ = D.unpack_bits(w, dims)
        d2, near = D.sweep(occ, md)
        if occ.size <= 50000:
            b2, bnear = D.brute(occ, md)
            assert np.array_equal(d2, b2) and np.array_equal(near, bnear), name
        if occ.any():
            edt = np.rint(ndi.distance_transform_edt(~occ) ** 2).astype(np.int64)
            assert np.array_equal(d2, np.where(edt <= md * md, edt, D.NONE16).astype(np.uint16)), name
        else:
            assert (d2 == D.NONE16).all() and (near == D.NONE32).all(), name
        # the nearest source attains the distance
        some = d2 != D.NONE16
        n = near[some].astype(np.int64)
        cells = np.flatnonzero(some.reshape(-1))
        off = [(n // s % m) - (cells // s % m) for s, m in ((1, dims[0]), (dims[0], dims[1]), (dims[0] * dims[1], dims[2]))]
        assert occ.reshape(-1)[n].all() and np.array_equal(off[0] ** 2 + off[1] ** 2 + off[2] ** 2, d2[some].astype(np.int64)), name


def test_the_scenes_are_what_they_were_built_to_be():
    dims, w, md = one_source()
    d2, near = D.brute(D.unpack_bits(w, dims), md)
    at = lambda a, b, c: int(d2[8 + c, 8 + b, 8 + a])
    assert (at(2, 3, 6), at(4, 4, 4), at(0, 0, 7), at(5, 5, 0), at(0, 1, 7), at(0, 0, 0)) == (49, 48, 49, D.NONE16, D.NONE16, 0)
    assert at(-2, -3, -6) == 49 and at(-7, 0, 0) == 49 and at(-8, 0, 0) == D.NONE16
    B = 8 + 64 * (8 + 16 * 8)
    assert set(near[d2 != D.NONE16].tolist()) == {B} and int((d2 != D.NONE16).sum()) == 1419  # the lattice points of the ball of radius 7
    # the row's end: the cell after the source in the words is 63 cells and a row away
    dims, w, md, _ = scenes()["wrap"]
    d2 = D.brute(D.unpack_bits(w, dims), md)[0]
    assert d2[0, 1, 0] == D.NONE16 and d2[0, 0, 62] == 1 and d2[0, 1, 63] == 1 and d2[1, 0, 63] == 1
    # the lattice: every cell midway between two sources names the one with the smaller bit number
    dims, w, md = lattice()
    d2, near = D.brute(D.unpack_bits(w, dims), md)
    assert d2[0, 0, 2] == 4 and near[0, 0, 2] == 0 and d2[2, 2, 2] == 12 and near[2, 2, 2] == 0 and near[0, 0, 3] == 4
    # rule 4's pair and the clamp; the counts
    assert [want(n)["r2"] for n in ("odd_0.01_md5", "odd_0.01_md5_below", "odd_0.3_md65", "odd_0.0005_md130")] == [9, 8, 0, 130 * 130]
    a, b = want("odd_0.01_md5"), want("odd_0.01_md5_below")
    assert a["counts"][3] - b["counts"][3] == int((a["dist2"] == 9).sum()) > 0 and np.array_equal(a["dist2"], b["dist2"])
    for name in scenes():
        r, n = want(name), int(np.prod(scenes()[name][0]))
        bits = np.unpackbits(r["inflated"].view(np.uint8), bitorder="little").astype(bool)
        assert sum(r["counts"][:3]) == n and r["counts"][3] == int(bits.sum()) >= r["counts"][0], name
        assert np.array_equal(bits, r["dist2"] <= r["r2"]) and np.array_equal(r["dist2"] == 0, D.unpack_bits(scenes()[name][1], scenes()[name][0]).reshape(-1)), name
        assert np.array_equal(np.isinf(r["clearance"]), r["dist2"] == D.NONE16) and np.array_equal(r["nearest"] == D.NONE32, r["dist2"] == D.NONE16), name
    assert want("64_zero")["counts"] == [0, 0, 64, 0] and want("64_ones")["counts"] == [64, 0, 0, 64]
    assert want("odd_0.0005_md130")["counts"][3] == want("odd_0.0005_md130")["counts"][0] + want("odd_0.0005_md130")["counts"][1]  # the clamp inflates all that is reached
    assert want("odd_0.01_md5")["counts"][2] > 0 and want("big_corners_md254")["counts"][2] == 0


# variant -> (scene, cells whose dist2 or nearest changes)
MISREADINGS = {"tie_larger": ("lattice", 1695), "lt_cap": ("one_source", 54), "cube": ("one_source", 1956), "chessboard": ("one_source", 3332),
               "manhattan": ("one_source", 1376), "left_only": ("one_source", 635), "none_sources": ("one_source", 1), "swap_d1_d2": ("swap", 170),
               "row_wrap": ("wrap", 3)}  # lt_cap: the 54 lattice points at exactly 49; cube: 15^3 - 1419; left_only: (1419 - 149) / 2


def test_every_misreading_of_the_rules_changes_a_stated_scene():
    swap_dims = (64, 5, 3)
    sc = {"lattice": lattice(), "one_source": one_source(), "wrap": scenes()["wrap"][:3], "swap": (swap_dims, bits_of([(10, 3, 1)], swap_dims), 9)}
    assert set(MISREADINGS) == set(D.VARIANTS)
    for v, (name, changed) in MISREADINGS.items():
        dims, w, md = sc[name]
        occ = D.unpack_bits(w, dims)
        a, b = D.brute(occ, md), D.brute(occ, md, variant=v)
        got = int(((a[0] != b[0]) | (a[1] != b[1])).sum())
        print(v, name, got)
        assert got == changed, (v, got)
    dims, w, md = sc["wrap"]
    assert D.brute(D.unpack_bits(w, dims), md, variant="row_wrap")[0][0, 1, 0] == 1


def test_pure_entries_and_refusals_without_a_context():
    from stereo_vo_amd import api
    lib = api.lib()
    p = api.voxel_distance_default_params(0.1)
    assert (p.max_dist, p.inflate_radius) == (32, 0.0) and C.sizeof(api.VoxelDistanceParams) == 8 and C.sizeof(api.VoxelDistanceOut) == 32
    assert api.VoxelSphere == D.Sphere and api.VoxelSphereHit == D.SphereHit and api.VoxelSphere.itemsize == 16 and api.VoxelSphereHit.itemsize == 16
    assert api.VOXEL_SPHERE_CODE == ("FREE", "COLLIDES", "OUTSIDE", "REJECTED") and api.VOXEL_DISTANCE_NONE16 == D.NONE16
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(api.SvoError):
            api.voxel_distance_default_params(bad)
    assert lib.svo_voxel_distance_default_params(C.c_float(0.1), None) == -1
    for dims in [sc[0] for sc in scenes().values()] + [(512, 128, 512), (1024, 1024, 1024), (2048, 2048, 256)]:
        n = dims[0] * dims[1] * dims[2]
        assert api.voxel_distance_bytes(dims) == 2 * n and api.voxel_distance_workspace_bytes(dims) == 3 * n <= 4 * n
        assert api.voxel_distance_workspace_bytes(dims, True) == 6 * n <= 8 * n
    assert api.voxel_distance_workspace_bytes((2048, 2048, 256), True) == 6 * 2 ** 30 > 2 ** 32  # size_t, not int
    for bad in ((0, 1, 1), (32, 1, 1), (96, 1, 1), (64, 0, 1), (64, 1, 2049), (2048, 1024, 1024)):
        with pytest.raises(api.SvoError):
            api.voxel_distance_bytes(bad)
        with pytest.raises(api.SvoError):
            api.voxel_distance_workspace_bytes(bad, True)
    n = C.c_size_t(7)
    i3 = (C.c_int * 3)(64, 1, 1)
    assert lib.svo_voxel_distance_bytes(None, C.byref(n)) == -1 and n.value == 0 and lib.svo_voxel_distance_bytes(i3, None) == -1
    n = C.c_size_t(7)
    assert lib.svo_voxel_distance_workspace_bytes(None, 0, C.byref(n)) == -1 and n.value == 0 and lib.svo_voxel_distance_workspace_bytes(i3, 0, None) == -1
    buf = (C.c_double * 16)()
    out = api.VoxelDistanceOut(C.addressof(buf), None, None, None)
    assert lib.svo_voxel_occupancy_distance_dev(None, buf, i3, C.byref(p), buf, C.byref(out), None) == -1
    assert lib.svo_voxel_distance_query_dev(None, buf, i3, i3, buf, 1, buf, None) == -1
    assert lib.svo_voxel_distance_query(None, buf, i3, i3, buf, 1, buf, None) == -1
    assert lib.svo_voxel_map_distance(None, 1, i3, i3, C.byref(p), C.byref(out), None) == -1


# ----------------------------------------------------------------------------------------------------- the query
def centre(j, frac=(0.5, 0.5, 0.5)):
    return tuple(F32((ORIGIN[r] + j[r] + frac[r]) * VS) for r in range(3))


@functools.lru_cache(maxsize=None)
def query_scene():
    """(spheres, the wanted code of each constructed one) over the field of "odd_0.01_md5" at ORIGIN."""
    dims = scenes()["odd_0.01_md5"][0]
    d2 = want("odd_0.01_md5")["dist2"].reshape(dims[2], dims[1], dims[0])
    cell = lambda v: tuple(int(x) for x in np.argwhere(d2 == v)[0][::-1])  # the first cell of that dist2, as (j0, j1, j2)
    nine, src, none = cell(9), cell(0), cell(D.NONE16)
    down = lambda v: F32(np.nextafter(F32(v), F32(-np.inf)))
    face = F32((ORIGIN[0] + 40) * VS)  # the face between j0 = 39 and 40
    rows = [(*centre(nine), 1.5, D.COLLIDES), (*centre(nine), BELOW_1_5, D.FREE),                # rc^2 exactly 9, and just less
            (*centre(src), 0.0, D.COLLIDES), (*centre(src), -0.0, D.COLLIDES), (*centre(nine), 0.0, D.FREE),
            (face, *centre((40, 4, 6))[1:], 0.0, None), (down(face), *centre((40, 4, 6))[1:], 0.0, None),  # a voxel face and one ulp below it
            (F32(-524280.0), 0.0, 0.0, 1.0, D.OUTSIDE), (down(-524280.0), 0.0, 0.0, 1.0, D.REJECTED),  # q = -1048560 is in, the float below is not
            (0.0, F32(524280.0), 0.0, 1.0, D.REJECTED), (0.0, down(524280.0), 0.0, 1.0, D.OUTSIDE),    # q = 1048560 is out, the float below is in
            (*centre(nine), float("nan"), D.REJECTED), (*centre(nine), float("inf"), D.REJECTED), (*centre(nine), -1e-30, D.REJECTED),
            (float("nan"), 0.0, 0.0, 1.0, D.REJECTED), (0.0, float("inf"), 0.0, 1.0, D.REJECTED), (0.0, 0.0, float("-inf"), 1.0, D.REJECTED),
            (*centre((-1, 4, 6)), 1.0, D.OUTSIDE), (*centre((128, 4, 6)), 1.0, D.OUTSIDE), (*centre((5, 9, 6)), 1.0, D.OUTSIDE), (*centre((5, 4, -1)), 1.0, D.OUTSIDE),
            (*centre((0, 0, 0), (0.0, 0.0, 0.0)), 0.25, None), (*centre((127, 8, 12), (0.99, 0.99, 0.99)), 0.25, None),
            (*centre(none), 100.0, D.FREE), (*centre(none), 3.0e4, D.FREE), (*centre(none), 4.0e4, D.COLLIDES)]  # beyond max_dist: 65,536 voxels collide
    rng = np.random.default_rng(21)
    for _ in range(1025 - len(rows)):
        j = rng.uniform(-2, [dims[0] + 2, dims[1] + 2, dims[2] + 2])
        rows.append((*((np.asarray(ORIGIN) + j) * VS).astype(F32), F32(rng.uniform(0, 3.0)), None))
    s = np.zeros(len(rows), D.Sphere)
    for i, r in enumerate(rows):
        s[i] = r[:4]
    return s, [r[4] for r in rows], (nine, src, none)


def test_the_query_rule_on_constructed_spheres():
    s, codes, (nine, src, none) = query_scene()
    dims = scenes()["odd_0.01_md5"][0]
    f = want("odd_0.01_md5")
    hits, counts = D.query(f["dist2"], ORIGIN, dims, s, VS)
    for i, c in enumerate(codes):
        assert c is None or hits["code"][i] == c, (i, s[i], hits[i])
    B = lambda j: j[0] + dims[0] * (j[1] + dims[1] * j[2])
    assert hits["cell"][0] == hits["cell"][1] == B(nine) and hits["dist2"][0] == 9 and hits["clearance"][0] == F32(1.5)
    assert hits["cell"][5] == B((40, 4, 6)) and hits["cell"][6] == B((39, 4, 6))
    assert hits["cell"][21] == 0 and hits["cell"][22] == dims[0] * dims[1] * dims[2] - 1
    assert hits["cell"][23] == B(none) and hits["dist2"][23] == D.NONE32 and np.isinf(hits["clearance"][23])
    out = np.isin(hits["code"], (D.OUTSIDE, D.REJECTED))
    assert (hits["cell"][out] == D.NONE32).all() and (hits["dist2"][out] == D.NONE32).all() and np.isinf(hits["clearance"][out]).all()
    assert counts[0] == 1025 == sum(counts[1:5]) and min(counts[1:]) >= 3 and np.array_equal(hits["clearance"][~out].view(np.uint32),
                                                                                              f["clearance"][hits["cell"][~out]].view(np.uint32))
    assert D.query(f["dist2"], ORIGIN, dims, s[:0], VS)[1] == [0] * 6


def _scene_file(path, dims, origin, md, rad, vs, words, f, spheres=None):
    s = np.zeros(0, D.Sphere) if spheres is None else spheres
    hits, qc = D.query(f["dist2"], origin, dims, s, vs)
    with open(path, "wb") as fh:
        fh.write(struct.pack("<8i2f", *dims, *origin, md, len(s), vs, rad) + np.ascontiguousarray(words, np.uint64).tobytes() + f["dist2"].tobytes() +
                 f["nearest"].tobytes() + f["clearance"].tobytes() + f["inflated"].tobytes() + np.array(f["counts"], np.uint64).tobytes() + s.tobytes() +
                 hits.tobytes() + np.array(qc, np.uint64).tobytes())
    return str(path)


def test_voxel_distance_host_logic_under_sanitizers(tmp_path):
    """host/voxel_distance.h on the CPU under ASan + UBSan: every refusal at its boundary with code, message and order, R2, the
    defaults, the sizes and the launch geometry, and - from files of the restatement's numbers - the three passes in both forms over
    a dirty workspace of the stated size, and the query, for a handful of the scenes."""
    files = []
    for name in ("64_ends_md1", "64_random_md254", "wrap", "odd_0.01_md5", "odd_0.3_md65", "odd_corners_md254", "odd_words_md64", "long_md65", "long_md254",
                 "long_0.0005_md254", "odd_zero_md130"):
        dims, w, md, rad = scenes()[name]
        files.append(_scene_file(tmp_path / (name + ".bin"), dims, ORIGIN, md, rad, VS, w, want(name), query_scene()[0] if name == "odd_0.01_md5" else None))
    dims, w, md = lattice()
    files.append(_scene_file(tmp_path / "lattice.bin", dims, (0, 0, 0), md, 0.37, 0.1, w, D.field(w, dims, md, 0.37, 0.1, route="brute")))
    out = _run_sanitized(tmp_path, "voxel_distance_args_test", "voxel distance args ok", *files)
    assert out.count(" cells, ") == len(files) and "1025 spheres" in out


# ===================================================================================================== GPU
def _bits(words):
    """The volume between two guards of all-ones words, which would be sources if read."""
    import torch
    t, p, g = _guarded(len(words), torch.int64, -1)
    t[g:-g] = torch.from_numpy(np.ascontiguousarray(words).view(np.int64).copy()).cuda()
    return t, p, g


def _field_call(vm, bits, dims, md, rad, nearest=True, clearance=True, inflated=True, counts=True):
    """One distance call into sentinel-filled guarded outputs over a dirty workspace: a dict like the restatement's."""
    import torch
    from stereo_vo_amd import api
    before, stats = TA._frozen(vm)
    n = dims[0] * dims[1] * dims[2]
    bt, bp, bg = bits
    d2 = _guarded(n, torch.int16, SENT16)
    nr = _guarded(n, torch.int32, SENT32)
    cl = _guarded(n, torch.int32, SENT32)
    inf = _guarded(n // 64, torch.int64, SENT)
    ct = _guarded(4, torch.int64, SENT)
    wsb = api.voxel_distance_workspace_bytes(dims, nearest)
    assert wsb % 8 == 0
    ws = _guarded(wsb // 8, torch.int64, SENT)
    torch.cuda.synchronize()
    vm.distance(bp, dims, workspace_ptr=ws[1], dist2_ptr=d2[1], nearest_ptr=nr[1] if nearest else None, clearance_ptr=cl[1] if clearance else None,
                inflated_ptr=inf[1] if inflated else None, counts_ptr=ct[1] if counts else None, max_dist=md, inflate_radius=rad)
    vm.ctx.sync()
    _unguard(ws[0], ws[2], SENT)  # the workspace's guards stand
    got = {"dist2": _unguard(d2[0], d2[2], SENT16).view(np.uint16), "ptr": d2[1], "hold": (d2, inf), "inflated_ptr": inf[1]}
    for key, on, buf, sent, view in (("nearest", nearest, nr, SENT32, np.uint32), ("clearance", clearance, cl, SENT32, np.float32), ("inflated", inflated, inf, SENT, np.uint64),
                                     ("counts", counts, ct, SENT, np.uint64)):
        if on:
            got[key] = _unguard(buf[0], buf[2], sent).view(view)
        else:
            assert (buf[0].cpu().numpy() == sent).all(), key
    if counts:
        got["counts"] = got["counts"].tolist()
    a = bt.cpu().numpy()
    assert (a[:bg] == -1).all() and (a[-bg:] == -1).all()
    after, stats2 = TA._frozen(vm)
    assert all(np.array_equal(before[k], after[k]) for k in before) and stats2 == stats
    return got


def _assert_field(got, w, what):
    for k in ("dist2", "nearest", "inflated"):
        if k in got:
            bad = np.flatnonzero(got[k] != w[k])
            assert not len(bad), (what, k, len(bad), bad[:8].tolist(), got[k][bad[:8]].tolist(), w[k][bad[:8]].tolist())
    if "clearance" in got:
        assert np.array_equal(got["clearance"].view(np.uint32), w["clearance"].view(np.uint32)), (what, "clearance")
    if "counts" in got:
        assert got["counts"] == w["counts"], (what, got["counts"], w["counts"])


SMALL = [n for n in scenes() if int(np.prod(scenes()[n][0])) <= 20000]
LARGE = [n for n in scenes() if n not in SMALL]


@pytest.mark.gpu
def test_the_small_volumes_with_every_output(ctx):
    vm = T._map(ctx, VS, 8)
    ctx.profile_select("voxel_distance")
    for name in SMALL:
        dims, w, md, rad = scenes()[name]
        _assert_field(_field_call(vm, _bits(w), dims, md, rad), want(name), name)
    assert ctx.profile_read()[1] == len(SMALL)
    ctx.profile_select(None)
    vm.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", LARGE)
def test_the_larger_volumes(ctx, name):
    vm = T._map(ctx, VS, 8)
    dims, w, md, rad = scenes()[name]
    _assert_field(_field_call(vm, _bits(w), dims, md, rad), want(name), name)
    _assert_field(_field_call(vm, _bits(w), dims, md, rad, nearest=False), want(name), name + " without nearest")
    vm.close()


@pytest.mark.gpu
def test_a_repeated_call_and_each_optional_output_left_out(ctx):
    vm = T._map(ctx, VS, 8)
    for name in ("odd_0.01_md5", "odd_0.3_md65", "long_md130"):
        dims, w, md, rad = scenes()[name]
        bits = _bits(w)
        first, second = _field_call(vm, bits, dims, md, rad), _field_call(vm, bits, dims, md, rad)
        assert all(np.array_equal(first[k], second[k]) for k in ("dist2", "nearest", "inflated")) and first["clearance"].tobytes() == second["clearance"].tobytes()
        assert first["counts"] == second["counts"]
        _assert_field(first, want(name), name)
        for off in ({"nearest": False}, {"clearance": False}, {"inflated": False}, {"counts": False}, {"nearest": False, "clearance": False, "inflated": False},
                    {"nearest": False, "clearance": False, "inflated": False, "counts": False}):
            _assert_field(_field_call(vm, bits, dims, md, rad, **off), want(name), (name, off))
    vm.close()


def _query_call(vm, dist2_ptr, origin, dims, spheres, hits=True, counts=True):
    import torch
    n = len(spheres)
    ht, hp, hg = _guarded(4 * n, torch.int32, SENT32)
    nt, np_, ng = _guarded(6, torch.int64, SENT)
    t = torch.from_numpy(np.ascontiguousarray(spheres).view(np.int32).reshape(-1, 4).copy()).cuda() if n else None
    torch.cuda.synchronize()
    vm.distance_query(dist2_ptr, origin, dims, t.data_ptr() if n else None, n, hits_ptr=hp, counts_ptr=np_ if counts else None)
    vm.ctx.sync()
    got = _unguard(nt, ng, SENT).view(np.uint64).tolist() if counts else None
    if not counts:
        assert (nt.cpu().numpy() == SENT).all()
    return _unguard(ht, hg, SENT32).view(D.SphereHit), got


@pytest.mark.gpu
def test_the_query_over_all_codes_by_both_entries(ctx):
    from stereo_vo_amd import api
    vm = T._map(ctx, VS, 8)
    dims, w, md, rad = scenes()["odd_0.01_md5"]
    f = _field_call(vm, _bits(w), dims, md, rad)
    _assert_field(f, want("odd_0.01_md5"), "field")
    s = query_scene()[0]
    wh, wc = D.query(want("odd_0.01_md5")["dist2"], ORIGIN, dims, s, VS)
    ctx.profile_select("voxel_distance_query")
    for n in (1025, 257, 64, 1):
        hits, counts = _query_call(vm, f["ptr"], ORIGIN, dims, s[:n])
        w = D.query(want("odd_0.01_md5")["dist2"], ORIGIN, dims, s[:n], VS)
        assert hits.tobytes() == w[0].tobytes() and counts == w[1], n
    hits, counts = _query_call(vm, f["ptr"], ORIGIN, dims, s, counts=False)
    assert hits.tobytes() == wh.tobytes()
    hits, counts = _query_call(vm, f["ptr"], ORIGIN, dims, s[:0])
    assert len(hits) == 0 and counts == [0] * 6
    assert ctx.profile_read()[1] == 6
    ctx.profile_select(None)
    hh, hc = vm.distance_query_host(f["ptr"], ORIGIN, dims, s)
    assert hh.tobytes() == wh.tobytes() and [hc[k] for k in api.DISTANCE_QUERY_COUNTS] == wc
    hh, hc = vm.distance_query_host(f["ptr"], ORIGIN, dims, s[:0])
    assert len(hh) == 0 and sum(hc.values()) == 0
    vm.close()


@pytest.mark.gpu
def test_rays_over_the_inflated_volume_are_swept_sphere_tests(ctx):
    """The device's inflated bits go into the sight lines' entry as they are: the records are voxel_rays_ref's over the restatement's
    inflated bits, with coarse NULL and with coarse built from the inflated volume."""
    R = TR.R
    for words, dims, origin, vs, rad, md, seed in ((TR.slab_words(), TR.SLAB_DIMS, TR.SLAB_ORIGIN, TR.SLAB_VS, 0.25, 8, 31),
                                                   (random_words((128, 9, 13), 0.01, 2), (128, 9, 13), ORIGIN, TR.VS, 0.5, 5, 32)):
        vm = T._map(ctx, vs, 8)
        f = _field_call(vm, _bits(words), dims, md, rad)
        w = D.field(words, dims, md, rad, vs)
        _assert_field(f, w, dims)
        assert w["counts"][3] > w["counts"][0] > 0
        rays = TR.random_rays(dims, origin, 300, seed, vs=vs)
        wh, wc = R.rays(w["inflated"], origin, dims, rays, 1, vs)
        thin = R.rays(words, origin, dims, rays, 1, vs)[1]
        assert wc[0] > thin[0]  # the inflated volume stops rays that pass the thin one
        coarse, ct, cp = TR._coarse_call(vm, f["inflated_ptr"], dims)
        assert np.array_equal(coarse, R.coarse_np(w["inflated"], dims))
        for c in (None, cp):
            hits, counts = TR._rays_call(vm, f["inflated_ptr"], c, origin, dims, rays, 1)
            TR._assert_hits(hits, wh, (dims, c))
            assert counts == wc
        vm.close()


HOST_DIMS = (128, 64, 128)


@pytest.mark.gpu
@pytest.mark.parametrize("vs,lg", TA.SIZES)
def test_the_host_entry_against_the_dev_entry_through_a_filled_map(ctx, vs, lg):
    from stereo_vo_amd import api
    vm = TA._build(ctx, [("insert", TN.corner(10), TA._m(TA.TRUTH))], vs, 0.0, lg)
    m12 = TA._m(TA.TRUTH)
    origin = TR.R.origin_of((m12[3], m12[7], m12[11]), vs, HOST_DIMS)
    words, occ, d, bt, bp = _occupancy_call(vm, origin, HOST_DIMS, 1)
    assert occ[0] > 100
    md, rad = 12, 3.0 * vs
    w = D.field(words, HOST_DIMS, md, rad, vs)
    print("corner", vs, "counts", w["counts"], "R2", w["r2"])
    assert w["counts"][1] > 1000 and w["counts"][3] > w["counts"][0]
    _assert_field(_field_call(vm, _bits(words), HOST_DIMS, md, rad), w, ("dev", vs))
    h = vm.distance_host(origin, HOST_DIMS, max_dist=md, inflate_radius=rad)
    h["counts"] = [h["counts"][k] for k in api.DISTANCE_COUNTS]
    _assert_field({k: (v.reshape(-1) if k != "counts" else v) for k, v in h.items()}, w, ("host", vs))
    h = vm.distance_host(origin, HOST_DIMS, max_dist=md, inflate_radius=rad, nearest=False, clearance=False, inflated=False)
    assert sorted(h) == ["counts", "dist2"] and np.array_equal(h["dist2"].reshape(-1), w["dist2"])
    vm.close()


@pytest.mark.gpu
def test_bad_arguments_launch_nothing_and_leave_the_map_usable(ctx):
    import torch
    from stereo_vo_amd import api
    lib = ctx.L
    pts, m = TR.slab_table()
    vm = TA._build(ctx, [("insert", pts[:500], m)], TR.SLAB_VS, 0.0, 12)
    dims = (64, 8, 8)
    n = 64 * 8 * 8
    bt, bp, bg = _guarded(n // 64, torch.int64, SENT)
    wt, wp, wg = _guarded(6 * n // 8, torch.int64, SENT)
    dt, dp, dg = _guarded(n, torch.int16, SENT16)
    nt, np_, ng = _guarded(n, torch.int32, SENT32)
    ft, fp, fg = _guarded(n, torch.int32, SENT32)
    it, ip, ig = _guarded(n // 64, torch.int64, SENT)
    kt, kp, kg = _guarded(6, torch.int64, SENT)
    st, sp, sg = _guarded(4 * 5, torch.int32, SENT32)
    ht, hp, hg = _guarded(4 * 5, torch.int32, SENT32)
    torch.cuda.synchronize()
    I3 = lambda *v: (C.c_int * 3)(*v)
    o3, d3 = I3(0, 0, 0), I3(*dims)
    host = np.zeros(n, np.uint16)
    hostp = host.ctypes.data

    def P(md=32, rad=0.0):
        return C.byref(api.VoxelDistanceParams(md, rad))

    def O(d2=None, nr=None, cl=None, inf=None):
        return C.byref(api.VoxelDistanceOut(dp if d2 is None else d2, np_ if nr is None else nr, fp if cl is None else cl, ip if inf is None else inf))

    fd = lambda b=None, d=d3, p=None, ws=None, o=None, k=None: lib.svo_voxel_occupancy_distance_dev(
        vm.h, bp if b is None else b, d, P() if p is None else p, wp if ws is None else ws, O() if o is None else o, kp if k is None else k)
    qy = lambda f=None, o=o3, d=d3, s=None, nn=5, h=None, k=None: lib.svo_voxel_distance_query_dev(
        vm.h, dp if f is None else f, o, d, sp if s is None else s, nn, hp if h is None else h, kp if k is None else k)
    hd = lambda mc=1, o=o3, d=d3, p=None, out=None: lib.svo_voxel_map_distance(
        vm.h, mc, o, d, P() if p is None else p, C.byref(api.VoxelDistanceOut(hostp, None, None, None)) if out is None else out, None)
    nul = C.c_void_p(0)
    calls = [(lambda: fd(p=nul), "null params"), (lambda: fd(p=P(md=0)), "max_dist"), (lambda: fd(p=P(md=255)), "max_dist"), (lambda: fd(p=P(rad=float("nan"))), "inflate_radius"),
             (lambda: fd(p=P(rad=float("inf"))), "inflate_radius"), (lambda: fd(p=P(rad=-1.0)), "inflate_radius"), (lambda: fd(d=None), "null dims"),
             (lambda: fd(d=I3(64, 0, 1)), "dims outside"), (lambda: fd(d=I3(96, 1, 1)), "multiple of 64"), (lambda: fd(d=I3(2048, 1024, 1024)), "2^30"),
             (lambda: fd(b=0), "null bits"), (lambda: fd(b=bp + 4), "bits must be 8-byte"), (lambda: fd(ws=0), "null workspace"), (lambda: fd(ws=wp + 4), "workspace must be 8-byte"),
             (lambda: fd(o=nul), "null out"), (lambda: fd(o=C.byref(api.VoxelDistanceOut(None, np_, fp, ip))), "null dist2"), (lambda: fd(o=O(d2=dp + 1)), "dist2 must be 2-byte"),
             (lambda: fd(o=O(nr=np_ + 2)), "nearest must be 4-byte"), (lambda: fd(o=O(cl=fp + 2)), "clearance must be 4-byte"), (lambda: fd(o=O(inf=ip + 4)), "inflated must be 8-byte"),
             (lambda: fd(k=kp + 4), "counts must be 8-byte"), (lambda: fd(p=P(md=0), d=None), "max_dist"), (lambda: fd(b=0, ws=0), "null bits"),
             (lambda: fd(ws=wp + 4, o=nul), "workspace must be"), (lambda: fd(o=O(d2=dp + 1, nr=np_ + 2)), "dist2 must be"), (lambda: fd(o=O(inf=ip + 4), k=kp + 4), "inflated must be"),
             (lambda: qy(nn=-1), "n must not"), (lambda: qy(nn=(1 << 20) + 1), "2^20"), (lambda: qy(o=None), "null origin"), (lambda: qy(o=I3(0, 1 << 20, 0)), "origin outside"),
             (lambda: qy(d=None), "null dims"), (lambda: qy(d=I3(32, 1, 1)), "multiple of 64"), (lambda: qy(f=0), "null dist2"), (lambda: qy(f=dp + 1), "dist2 must be 2-byte"),
             (lambda: qy(h=0), "null hits"), (lambda: qy(h=hp + 8), "hits must be 16-byte"), (lambda: qy(k=kp + 4), "counts must be 8-byte"), (lambda: qy(s=0), "null spheres"),
             (lambda: qy(s=sp + 8), "spheres must be 16-byte"), (lambda: qy(nn=-1, o=None), "n must not"), (lambda: qy(h=hp + 8, k=kp + 4), "hits must be"),
             (lambda: lib.svo_voxel_distance_query(vm.h, dp, o3, d3, None, 5, hostp, None), "null spheres"),
             (lambda: lib.svo_voxel_distance_query(vm.h, dp, o3, d3, hostp, 5, None, None), "null hits"),
             (lambda: hd(mc=0), "min_count"), (lambda: hd(p=nul), "null params"), (lambda: hd(p=P(md=255)), "max_dist"), (lambda: hd(o=None), "null origin"),
             (lambda: hd(d=None), "null dims"), (lambda: hd(out=nul), "null out"), (lambda: hd(out=C.byref(api.VoxelDistanceOut(None, None, None, None))), "null dist2")]
    assert len(calls) >= 45
    before, stats = TA._frozen(vm)
    for tag in ("voxel_distance", "voxel_distance_query", "voxel_occupancy"):
        ctx.profile_select(tag)
        for call, word in calls:
            assert call() == -1 and word in lib.svo_last_error(ctx.h).decode(), (word, lib.svo_last_error(ctx.h).decode())
        assert ctx.profile_read()[1] == 0
        ctx.profile_select(None)
    ctx.sync()
    for tt, s in ((bt, SENT), (wt, SENT), (dt, SENT16), (nt, SENT32), (ft, SENT32), (it, SENT), (kt, SENT), (st, SENT32), (ht, SENT32)):
        assert (tt.cpu().numpy() == s).all()
    assert not host.any()
    after, stats2 = TA._frozen(vm)
    assert all(np.array_equal(before[k], after[k]) for k in before) and stats2 == stats
    # the context and the map work
    words, occ, d, bt2, bp2 = _occupancy_call(vm, TR.SLAB_ORIGIN, TR.SLAB_DIMS, 1)
    assert occ == [500, 0]
    _assert_field(_field_call(vm, _bits(words), TR.SLAB_DIMS, 6, 0.2), D.field(words, TR.SLAB_DIMS, 6, 0.2, TR.SLAB_VS), "after the bad calls")
    vm.close()
