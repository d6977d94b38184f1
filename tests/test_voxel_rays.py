"""The voxel map sight lines (include/svo.h, "Voxel map sight lines"): the coarse volume, the rays and the camera form.

Without a GPU: the routes of the restatement (tests/voxel_rays_ref.py) agree on every scene, every misreading changes a stated
scene, the scenes reach all five codes and every axis, the slab property, the pure entries, and host/voxel_rays.h - the very
statements the kernels compile - under ASan + UBSan against the restatement's records.  On the GPU: the coarse words, every hit
record, the counts, disp16 and cell with == into sentinel-filled guarded buffers, with coarse NULL and with coarse given and the two
byte for byte, and the table's bytes and the map's counters before and after every call."""
import ctypes as C
import functools
import struct

import numpy as np
import pytest

import voxel_locate_ref as L
import voxel_ref as V
import voxel_rays_ref as R
import voxel_render_ref as VR
import test_voxel_align as TA
import test_voxel_map as T
import test_voxel_normals as TN
from test_host_sanitizers import _run_sanitized
from test_voxel_locate import _guarded, _unguard, _upload, _occupancy_call

F32 = np.float32
VS = 0.25  # the constructed scenes: a cell corner is exact in f32
SENT, SENT32, SENT16 = TA.SENT, 0x5A5A5A5A, 0x5A5A
NS = (0, 1, 63, 64, 65, 256, 257, 1025)
VOLUMES = {(64, 1, 1): (-5, 3, -2), (128, 9, 13): (-61, -3, -7), (128, 32, 128): (-64, -16, -64), (2048, 2, 2): (-1000, 0, -1)}
SLAB_DIMS, SLAB_ORIGIN, SLAB_VS, SLAB_CAM, SLAB_CENTRE, SLAB_WH = (128, 32, 128), (-64, -16, -64), 0.1, (60.0, 31.5, 23.5, 0.5), (0.03, 0.32, 0.01), (64, 48)
SLAB_WANT = (25, 23, 387)  # the first full row, the full rows, their pixels the splat render at max_radius 2 leaves FILTERED


# ----------------------------------------------------------------------------------------------------- scenes without a GPU
def fills(dims, seed):
    rng = np.random.default_rng(seed)
    nw = R.occupancy_words(dims)
    # sparse: three 8-blocks in a hundred hold anything, and those are half full: most of a walk is through empty blocks
    cd = R.coarse_dims(dims)
    blocks = rng.random((cd[2], cd[1], cd[0])) < 0.03
    cells = np.repeat(np.repeat(np.repeat(blocks, 8, 0), 8, 1), 8, 2)[:dims[2], :dims[1], :dims[0]] & (rng.random((dims[2], dims[1], dims[0])) < 0.5)
    out = {"random": rng.integers(0, 1 << 63, nw, dtype=np.uint64) ^ (rng.integers(0, 2, nw, dtype=np.uint64) << np.uint64(63)),
           "sparse": np.packbits(cells.reshape(-1).astype(np.uint8), bitorder="little").view(np.uint64),
           "ones": np.full(nw, ~np.uint64(0), np.uint64), "zero": np.zeros(nw, np.uint64)}
    if min(dims) > 8:
        out["bit777"], out["bit888"] = R.bits_of([(7, 7, 7)], dims), R.bits_of([(8, 8, 8)], dims)
    return out


def at(dims, origin, j, frac=(0.5, 0.5, 0.5), vs=VS):
    """The world position of the fraction `frac` of cell j: exact in f32 at VS."""
    o = [F32((origin[r] + j[r] + frac[r]) * vs) for r in range(3)]
    assert vs != VS or all(float(o[r]) == (origin[r] + j[r] + frac[r]) * vs for r in range(3))
    return o


def random_rays(dims, origin, n, seed, vs=VS, max_range=40.0):
    """Starts inside the volume (every fifth on a cell corner), directions normal, integer or with a zero component."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        j = [int(rng.integers(0, dims[r])) for r in range(3)]
        frac = (0.0, 0.0, 0.0) if i % 5 == 0 else tuple(rng.integers(0, 256, 3) / 256.0)
        d = rng.normal(size=3)
        if i % 7 == 0:
            d = rng.integers(-2, 3, 3).astype(float)
        if i % 11 == 0:
            d[int(rng.integers(0, 3))] = 0.0
        rows.append((*at(dims, origin, j, frac, vs), rng.random() * max_range, *d))
    return R.make_rays(rows)


AXES = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> (dims, origin, words, rays, min_step), all at VS."""
    out = {}
    for dims, origin in VOLUMES.items():
        tag = "x".join(str(d) for d in dims)
        mid = tuple(d // 2 for d in dims)
        last = tuple(d - 1 for d in dims)
        for fill, w in fills(dims, sum(dims)).items():
            w.setflags(write=False)
            rows = []
            for d in AXES:  # the three axis-aligned directions in both signs, from the middle, from cell 0 and from the last cell
                for j, frac in ((mid, (0.5, 0.5, 0.5)), ((0, 0, 0), (0.25, 0.0, 0.75)), (last, (0.0, 0.5, 0.5))):
                    rows.append((*at(dims, origin, j, frac), 1000.0, *d))
            for j in ((0, 0, 0), mid) if min(dims) > 8 else (mid,):  # triple ties from a cell corner, and a crossing at n = 0
                jj = (5, 5, 5) if j == (0, 0, 0) and min(dims) > 8 else j
                rows += [(*at(dims, origin, jj, (0.0, 0.0, 0.0)), 1000.0, 1, 1, 1), (*at(dims, origin, jj, (0.0, 0.0, 0.0)), 1000.0, -1, -1, -1),
                         (*at(dims, origin, jj, (0.0, 0.5, 0.5)), 1000.0, -1, 0.25, 0), (*at(dims, origin, jj, (0.5, 0.5, 0.5)), 1000.0, 2, -2, 2)]
            rows.append((*at(dims, origin, last, (0.5, 0.5, 0.5)), 1000.0, 1, 1, 1))  # in the last cell, stepping out at once
            for ms in (0, 1, 3):
                out[f"{tag}_{fill}_ms{ms}"] = (dims, origin, w, R.make_rays(rows), ms)
    dims, origin = (128, 32, 128), VOLUMES[(128, 32, 128)]
    f = fills(dims, sum(dims))
    # the range: a ray along +x from a cell's middle crosses at n = 128, that is 0.125 m at VS: max_range 0, one ulp below, at, one ulp above
    c = at(dims, origin, (60, 16, 64))
    edge = F32(0.125)
    rows = [(*c, mr, 1, 0, 0) for mr in (0.0, np.nextafter(edge, F32(0)), edge, np.nextafter(edge, F32(1)), 0.5)]
    rows += [(*c, mr, 3, 4, 0) for mr in (0.0, 0.3, 1.0)]
    out["range"] = (dims, origin, f["zero"], R.make_rays(rows), 1)
    # refused records
    bad = [(np.nan, 0, 0, 1, 1, 0, 0), (0, np.inf, 0, 1, 1, 0, 0), (0, 0, 0, np.nan, 1, 0, 0), (0, 0, 0, np.inf, 1, 0, 0), (0, 0, 0, 1, np.nan, 0, 0),
           (0, 0, 0, 1, 1, -np.inf, 0), (0, 0, 0, 1, 0, 0, 0), (0, 0, 0, 1, -0.0, 0.0, -0.0), (0, 0, 0, -1.0, 1, 0, 0), (0, 0, 0, -1e-30, 1, 0, 0),
           (0, 0, 0, 0.0, 1e-30, 0, 0), (0, 0, 0, 3e38, 0, 0, -3e38)]
    out["rejected"] = (dims, origin, f["random"], R.make_rays(bad), 1)
    # q_r at both ends of the limit: a volume that ends where the key range does
    lo, hi = F32(-262140.0), F32(262140.0)
    ends = [(lo, 1, 1, 5, 1, 0, 0), (np.nextafter(lo, F32(-np.inf)), 1, 1, 5, 1, 0, 0), (1, lo, 1, 5, 1, 0, 0), (1, 1, np.nextafter(lo, F32(-np.inf)), 5, 1, 0, 0)]
    out["q_low"] = ((64, 8, 8), (-(1 << 20), 0, 0), fills((64, 8, 8), 3)["sparse"], R.make_rays(ends), 0)
    ends = [(hi, 1, 1, 5, -1, 0, 0), (np.nextafter(hi, F32(0)), 1, 1, 5, -1, 0, 0), (1, 1, hi, 5, 1, 0, 0), (1, np.nextafter(hi, F32(0)), 1, 5, 1, 0, 0)]
    out["q_high"] = ((64, 8, 8), ((1 << 20) - 64, 0, 0), fills((64, 8, 8), 3)["sparse"], R.make_rays(ends), 0)
    # starts outside, one cell beyond each face
    rows = [(*at(dims, origin, j), 10.0, 1, 1, 1) for j in ((-1, 5, 5), (128, 5, 5), (5, -1, 5), (5, 32, 5), (5, 5, -1), (5, 5, 128), (-1000, 0, 0))]
    out["outside"] = (dims, origin, f["ones"], R.make_rays(rows), 0)
    # random rays in a sparse and in a dense volume: the lane and workgroup tails
    many = random_rays(dims, origin, max(NS), 7)
    for n in NS:
        out[f"n_{n}"] = (dims, origin, f["sparse"], many[:n], 1)
    out["dense_257"] = (dims, origin, f["random"], many[:257], 0)
    odd = (128, 9, 13)
    out["odd_dims_300"] = (odd, VOLUMES[odd], fills(odd, 9)["sparse"], random_rays(odd, VOLUMES[odd], 300, 8), 1)
    return out


@functools.lru_cache(maxsize=None)
def want(name, route="a"):
    dims, origin, w, rays, ms = scenes()[name]
    coarse = R.coarse_np(w, dims) if route == "skip" else None
    return R.rays(w, origin, dims, rays, ms, VS, route, coarse=coarse)


def slab_words():
    return R.bits_of([(j0, 20, j2) for j0 in range(128) for j2 in range(128)], SLAB_DIMS)


def slab_table():
    """The slab as a table: one record in the middle of every voxel of the layer, 10 m in front of the inserting camera."""
    i0, i2 = np.meshgrid(np.arange(-64, 64), np.arange(-64, 64))
    x, z = ((i0.ravel() + 0.5) * SLAB_VS).astype(F32), ((i2.ravel() + 0.5) * SLAB_VS + 10.0).astype(F32)
    pts = V.records(x, np.full(x.shape, F32(0.45)), z, np.full(x.shape, 0x40000000, np.uint32))
    return pts, TA.ident((0.0, 0.0, -10.0))


@functools.lru_cache(maxsize=None)
def slab_views():
    """(the ray view's disp16, cell and counts; the splat render's disp16 at max_radius 2), both from the slab's camera."""
    c2w = TA.ident(SLAB_CENTRE)
    w2c = TA.ident(tuple(-v for v in SLAB_CENTRE))
    rayed = R.raycast(slab_words(), SLAB_ORIGIN, SLAB_DIMS, *SLAB_WH, SLAB_CAM, c2w, 30.0, 1, SLAB_VS)
    pts, m = slab_table()
    table = V.insert_np(pts, m, SLAB_VS)
    assert np.array_equal(L.occupancy_np({"keys": table.keys, "ci": table.ci}, SLAB_ORIGIN, SLAB_DIMS, 1)[0], slab_words())
    splat = VR.render_np(table, *SLAB_WH, SLAB_CAM, w2c, SLAB_VS, 1, 2)[0]
    return rayed, splat


def test_the_routes_of_the_restatement_agree_on_every_scene():
    for name, (dims, origin, w, rays, ms) in scenes().items():
        a, ca = want(name)
        assert len(a) == len(rays) and sum(ca[:5]) == len(rays) and ca[5] == int(a["steps"].sum()), name
        b, cb = want(name, "b")
        assert a.tobytes() == b.tobytes() and ca == cb, name
    for name, (dims, origin, w, rays, ms) in scenes().items():
        k, ck = want(name, "skip")
        assert want(name)[0].tobytes() == k.tobytes() and want(name)[1] == ck, name
    for dims in VOLUMES:
        for fill, w in fills(dims, sum(dims)).items():
            assert np.array_equal(R.coarse_np(w, dims), R.coarse_py(w, dims)), (dims, fill)
    (disp, cell, counts), _ = slab_views()
    c2w = TA.ident(SLAB_CENTRE)
    for route in ("b", "skip"):
        d2, c2, n2 = R.raycast(slab_words(), SLAB_ORIGIN, SLAB_DIMS, *SLAB_WH, SLAB_CAM, c2w, 30.0, 1, SLAB_VS, route, coarse=R.coarse_np(slab_words(), SLAB_DIMS))
        assert np.array_equal(disp, d2) and np.array_equal(cell, c2) and counts == n2, route


def test_the_scenes_are_what_they_were_built_to_be():
    codes, axes = set(), set()
    for name in scenes():
        a, _ = want(name)
        codes |= set((a["status"] & 255).tolist())
        axes |= set((a["status"] >> 8).tolist())
    assert codes == {0, 1, 2, 3, 4} and axes == {0, 1, 2, 3}
    status = lambda name: [(int(s) & 255, int(s) >> 8) for s in want(name)[0]["status"]]
    # the range: max_range 0 and one ulp short of the crossing end at the first crossing; at it and beyond they pass it
    a, c = want("range")
    assert status("range")[:5] == [(R.RANGE, 0)] * 5 and a["steps"][:5].tolist() == [0, 0, 1, 1, 2] and a["dist"][:2].tolist() == [0.125, 0.125]
    assert a["dist"][2] == F32(0.375) and status("range")[5:] == [(R.RANGE, 1), (R.RANGE, 1), (R.RANGE, 0)] and a["steps"][5:].tolist() == [0, 2, 5]
    assert set(status("rejected")[:10]) == {(R.REJECTED, 3)} and (want("rejected")[0]["cell"][:10] == R.NO_CELL).all()
    assert [s[0] for s in status("rejected")[10:]] == [R.RANGE, R.HIT]  # a direction of 1e-30 and a range and a direction of 3e38 are rays
    assert [s[0] for s in status("q_low")] == [R.RANGE, R.REJECTED, R.OUTSIDE, R.REJECTED] and want("q_low")[0]["cell"][0] == 16 + 20 + 64 * (4 + 8 * 4)  # from j_0 = 16, 5 m on
    assert [s[0] for s in status("q_high")] == [R.REJECTED, R.RANGE, R.REJECTED, R.OUTSIDE]
    assert set(status("outside")) == {(R.OUTSIDE, 3)} and want("outside")[1] == [0, 0, 0, 7, 0, 0]
    # min_step with every bit set: a hit at the start, after one step, after three
    for ms in (0, 1, 3):
        a, c = want(f"128x32x128_ones_ms{ms}")
        st = status(f"128x32x128_ones_ms{ms}")
        inside = [i for i, s in enumerate(st) if s[0] == R.HIT]
        assert all(a["steps"][i] == ms for i in inside) and len(inside) >= 10 and all((st[i][1] == 3) == (ms == 0) for i in inside)
        assert ms == 0 or (st[-1] == (R.LEFT, 0) and a["steps"][-1] == 0)  # the last cell, stepping out at once: ties to axis 0
    # triple ties from a corner: (1, 1, 1) from cell (5, 5, 5) reaches the bit at (7, 7, 7) by x, y, z in turn: six steps, the last along z
    a, _ = want("128x32x128_bit777_ms1")
    i = 18
    assert (int(a["status"][i]), int(a["steps"][i]), int(a["cell"][i])) == (R.HIT | 2 << 8, 6, 7 + 128 * (7 + 32 * 7)) and a["dist"][i] == F32(np.sqrt(3.0) * 2 * VS)
    # (-1, -1, -1) from the same corner crosses all three axes at n = 0; a crossing at n = 0 has dist 0
    assert int(a["status"][i + 1]) & 255 == R.LEFT and int(a["steps"][i + 1]) == 15
    a, _ = want("128x32x128_ones_ms1")
    assert (int(a["status"][i + 2]), int(a["steps"][i + 2]), a["dist"][i + 2]) == (R.HIT | 0 << 8, 1, F32(0.0))  # x crossed at n = 0, from f_0 = 0
    # the long volume: 1,023 and 2,047 steps to the far face, every one jumped or walked
    a, c = want("2048x2x2_zero_ms1")
    assert a["steps"][0] == 1023 and a["steps"][1] == 2047 and int(a["status"][0]) == R.LEFT
    # the sparse scenes end in all of HIT, LEFT and RANGE, and the skipping walk jumps most of their cells
    _, c = want("n_1025")
    assert min(c[:3]) > 50 and c[5] > 20000, c
    dims, origin, w, rays, ms = scenes()["n_1025"]
    vol = R.Volume(w, dims, R.coarse_np(w, dims))
    jumped = steps = 0
    for ray in rays:
        s = R.setup_a(*R.widen(ray), VS, origin)
        if s is None:
            continue
        e, j, _ = R.walk_skip(s, vol, ms)
        jumped, steps = jumped + j, steps + e[3]
    print("n_1025: steps", steps, "jumped", jumped)
    assert steps == c[5] and jumped > steps // 2


def test_every_misreading_of_the_contract_changes_a_stated_scene():
    def differs(name, variant):
        dims, origin, w, rays, ms = scenes()[name]
        return R.rays(w, origin, dims, rays, ms, VS, "a", variant)[0].tobytes() != want(name)[0].tobytes()
    assert differs("128x32x128_bit777_ms1", "tie_largest")
    assert differs("range", "range_after")
    assert differs("128x32x128_zero_ms1", "neg_n")
    assert differs("n_257", "D_trunc")
    assert differs("128x32x128_ones_ms1", "min_step_off")
    for v in ("tie_largest", "range_after", "neg_n", "D_trunc", "min_step_off"):
        assert not differs("outside", v)
    (disp, cell, counts), _ = slab_views()
    d2 = R.raycast(slab_words(), SLAB_ORIGIN, SLAB_DIMS, *SLAB_WH, SLAB_CAM, TA.ident(SLAB_CENTRE), 30.0, 1, SLAB_VS, variant="z_ray")[0]
    assert not np.array_equal(disp, d2) and np.array_equal(disp == R.FILTERED, d2 == R.FILTERED)
    dims = (128, 9, 13)
    w = fills(dims, sum(dims))["bit777"]
    assert not np.array_equal(R.coarse_np(w, dims, VOLUMES[dims], "coarse_world"), R.coarse_np(w, dims))
    assert np.array_equal(R.coarse_np(w, dims, (-64, 8, 16), "coarse_world"), R.coarse_np(w, dims))  # an origin of whole blocks hides it
    assert len(R.VARIANTS) == 7


def test_a_full_layer_one_voxel_thick_stops_every_ray_where_the_splat_render_has_holes():
    """The render's KNOWN PROPERTY as a test.  A 6-connected walk cannot pass through a full layer, so every image row that has
    one hit is hit in every pixel; the splat render of the same voxels at max_radius 2 leaves holes in those rows.  What the
    restatement gives for the slab of the issue (64 x 48, focal 60, the camera 0.08 to 0.18 m above the layer): the 23 rows from
    row 25 down are full, and the render of one record in the middle of every voxel of the layer leaves 387 of their 1,472 pixels
    FILTERED."""
    (disp, cell, counts), splat = slab_views()
    hit = disp != R.FILTERED
    rows = np.flatnonzero(hit.any(axis=1))
    assert len(rows) > 0 and hit[rows].all()
    holes = int((splat[rows] == R.FILTERED).sum())
    print("slab: first row", rows[0], "rows", len(rows), "holes", holes, "counts", counts)
    assert holes >= 1 and (int(rows[0]), len(rows), holes) == SLAB_WANT
    assert counts[6] == hit.sum() == 64 * len(rows) and (cell[hit] != R.NO_CELL).all() and (cell[~hit] == R.NO_CELL).all()
    assert all(int(c) // 128 % 32 == 20 for c in cell[hit])  # every hit is a voxel of the layer


def test_pure_entries_and_refusals_without_a_context():
    from stereo_vo_amd import api
    lib = api.lib()
    p = api.voxel_raycast_default_params()
    assert (p.max_range, p.min_step) == (30.0, 1) and C.sizeof(api.VoxelRaycastParams) == 8
    assert api.VoxelRay == R.RAY and api.VoxelRayHit == R.HIT_T and api.VoxelRay.itemsize == 32 and api.VoxelRayHit.itemsize == 16
    assert api.VOXEL_RAY_STATUS == ("HIT", "LEFT", "RANGE", "OUTSIDE", "REJECTED") and api.RAYS_COUNTS[:5] == R.CODES
    assert lib.svo_voxel_raycast_default_params(None) == -1
    for dims in list(VOLUMES) + [(512, 128, 512), (1024, 1024, 1024), (64, 8, 9)]:
        assert api.voxel_occupancy_coarse_bytes(dims) == 8 * R.coarse_words(dims)
    assert api.voxel_occupancy_coarse_bytes((512, 128, 512)) == 8192
    for bad in ((0, 1, 1), (32, 1, 1), (96, 1, 1), (64, 0, 1), (64, 1, 2049), (2048, 1024, 1024)):
        with pytest.raises(api.SvoError):
            api.voxel_occupancy_coarse_bytes(bad)
    n = C.c_size_t(7)
    i3 = (C.c_int * 3)(64, 1, 1)
    assert lib.svo_voxel_occupancy_coarse_bytes(None, C.byref(n)) == -1 and n.value == 0 and lib.svo_voxel_occupancy_coarse_bytes(i3, None) == -1
    buf = (C.c_double * 16)()
    cam = api.CameraInfo(60.0, 31.5, 23.5, 0, 0, 0, 0, 0.5)
    assert lib.svo_voxel_occupancy_coarse_dev(None, buf, i3, buf) == -1
    assert lib.svo_voxel_occupancy_rays_dev(None, buf, None, i3, i3, buf, 1, 1, buf, None) == -1
    assert lib.svo_voxel_occupancy_rays(None, buf, None, i3, i3, buf, 1, 1, buf, None) == -1
    assert lib.svo_voxel_occupancy_raycast_dev(None, buf, None, i3, i3, 8, 8, C.byref(cam), buf, C.byref(p), buf, None, None) == -1
    assert lib.svo_voxel_occupancy_raycast_pose7_dev(None, buf, None, i3, i3, 8, 8, C.byref(cam), buf, C.byref(p), buf, None, None) == -1
    assert lib.svo_voxel_map_raycast(None, 1, i3, 8, 8, C.byref(cam), buf, C.byref(p), buf, None, None, None) == -1


def _scene_file(path, kind, dims, origin, min_step, vs, words, body, n=0, wh=(0, 0), max_range=0.0, cam=(1.0, 0.0, 0.0, 1.0), m12=TA.ident()):
    head = struct.pack("<11i2fi16d", kind, *dims, *origin, min_step, n, wh[0], wh[1], vs, max_range, 0, *cam, *[float(v) for v in m12])
    with open(path, "wb") as f:
        f.write(head + np.ascontiguousarray(words, np.uint64).tobytes() + R.coarse_np(words, dims).tobytes() + body)
    return str(path)


def test_voxel_rays_host_logic_under_sanitizers(tmp_path):
    """host/voxel_rays.h on the CPU under ASan + UBSan: every refusal at its boundary with code, message and order, the sizes and the
    launch geometry, and - from files of the restatement's numbers - each ray's set-up (p, D, L) and both walks' records, pixels
    and counts, for scenes of every kind and the slab's camera."""
    files = []
    names = ["128x32x128_bit777_ms1", "128x9x13_sparse_ms0", "64x1x1_random_ms3", "2048x2x2_zero_ms1", "2048x2x2_sparse_ms1", "128x32x128_ones_ms3", "range", "rejected",
             "q_low", "q_high", "outside", "n_1025", "dense_257", "odd_dims_300"]
    for name in names:
        dims, origin, w, rays, ms = scenes()[name]
        hits, counts = want(name)
        rows = np.zeros(len(rays), np.dtype([("p", np.int64, 3), ("L", np.int64, 3), ("D", np.int32, 3), ("ok", np.int32)]))
        for i, ray in enumerate(rays):
            s = R.setup_a(*R.widen(ray), VS, origin)
            if s is not None:
                rows[i] = (s.p, s.L, s.D, 1)
        body = rays.tobytes() + hits.tobytes() + rows.tobytes() + np.array(counts, np.uint64).tobytes()
        files.append(_scene_file(tmp_path / (name + ".bin"), 0, dims, origin, ms, VS, w, body, n=len(rays)))
    (disp, cell, counts), _ = slab_views()
    body = disp.tobytes() + cell.tobytes() + np.array(counts, np.uint64).tobytes()
    files.append(_scene_file(tmp_path / "slab.bin", 1, SLAB_DIMS, SLAB_ORIGIN, 1, SLAB_VS, slab_words(), body, wh=SLAB_WH, max_range=30.0, cam=SLAB_CAM,
                             m12=TA.ident(SLAB_CENTRE)))
    out = _run_sanitized(tmp_path, "voxel_rays_args_test", "voxel rays args ok", *files)
    assert f"({len(files)} files)" in out


# ===================================================================================================== GPU
def _coarse_call(vm, bits_ptr, dims):
    import torch
    ct, cp, cg = _guarded(R.coarse_words(dims), torch.int64, SENT)
    torch.cuda.synchronize()
    vm.occupancy_coarse(bits_ptr, dims, cp)
    vm.ctx.sync()
    return _unguard(ct, cg, SENT).view(np.uint64), ct, cp


def _rays_call(vm, bits_ptr, coarse_ptr, origin, dims, rays, min_step, counts=True, dev=None):
    """One rays call into guarded buffers: (the records, the six counts or None)."""
    import torch
    before, stats = TA._frozen(vm)
    n = len(rays)
    ht, hp, hg = _guarded(4 * n, torch.int32, SENT32)
    nt, np_, ng = _guarded(6, torch.int64, SENT)
    t = torch.from_numpy(np.ascontiguousarray(rays).view(np.int32).reshape(-1, 8).copy()).cuda() if dev is None and n else dev
    torch.cuda.synchronize()
    vm.rays(bits_ptr, origin, dims, t.data_ptr() if n else None, n, hits_ptr=hp, coarse_ptr=coarse_ptr, min_step=min_step, counts_ptr=np_ if counts else None)
    vm.ctx.sync()
    hits = _unguard(ht, hg, SENT32).view(R.HIT_T)
    got = _unguard(nt, ng, SENT).view(np.uint64).tolist() if counts else None
    if not counts:
        assert (nt.cpu().numpy() == SENT).all()
    after, stats2 = TA._frozen(vm)
    assert all(np.array_equal(before[k], after[k]) for k in before) and stats2 == stats
    return hits, got


def _assert_hits(got, wanted, what):
    bad = np.flatnonzero(got.view(np.uint32).reshape(-1, 4) != wanted.view(np.uint32).reshape(-1, 4)).tolist()
    assert not bad, (what, bad[:8], got[bad[0] // 4], wanted[bad[0] // 4])


@pytest.mark.gpu
def test_constructed_rays_by_both_walks(ctx):
    vm = T._map(ctx, VS, 8)
    ctx.profile_select("voxel_rays")
    calls = 0
    for name, (dims, origin, w, rays, ms) in scenes().items():
        bt, bp = _upload(w)
        coarse, ct, cp = _coarse_call(vm, bp, dims)
        assert np.array_equal(coarse, R.coarse_py(w, dims) if len(w) <= 4096 else R.coarse_np(w, dims)), name
        plain, pc = _rays_call(vm, bp, None, origin, dims, rays, ms)
        skip, sc = _rays_call(vm, bp, cp, origin, dims, rays, ms)
        calls += 2
        _assert_hits(plain, want(name)[0], name)
        assert plain.tobytes() == skip.tobytes() and pc == sc == want(name)[1], (name, pc, sc, want(name)[1])
    assert ctx.profile_read()[1] == calls
    ctx.profile_select("voxel_coarse")
    _coarse_call(vm, bp, dims)
    assert ctx.profile_read()[1] == 1
    ctx.profile_select(None)
    vm.close()


@pytest.mark.gpu
def test_a_repeated_call_no_rays_and_each_optional_output_left_out(ctx):
    import torch
    vm = T._map(ctx, VS, 8)
    dims, origin, w, rays, ms = scenes()["n_257"]
    bt, bp = _upload(w)
    coarse, ct, cp = _coarse_call(vm, bp, dims)
    again, ct2, cp2 = _coarse_call(vm, bp, dims)
    assert np.array_equal(coarse, again)
    dev = torch.from_numpy(np.ascontiguousarray(rays).view(np.int32).reshape(-1, 8).copy()).cuda()
    for c in (None, cp):
        first = _rays_call(vm, bp, c, origin, dims, rays, ms, dev=dev)
        second = _rays_call(vm, bp, c, origin, dims, rays, ms, dev=dev)
        assert first[0].tobytes() == second[0].tobytes() == want("n_257")[0].tobytes() and first[1] == second[1] == want("n_257")[1]
        _assert_hits(_rays_call(vm, bp, c, origin, dims, rays, ms, counts=False, dev=dev)[0], want("n_257")[0], "no counts")
        hits, counts = _rays_call(vm, bp, c, origin, dims, rays[:0], ms)  # n == 0: only the counts' memset
        assert len(hits) == 0 and counts == [0] * 6
        hh, hc = vm.rays_host(bp, origin, dims, rays, coarse_ptr=c, min_step=ms)
        assert hh.tobytes() == want("n_257")[0].tobytes() and [hc[k] for k in ("n_hit", "n_left", "n_range", "n_outside", "n_rejected", "n_steps")] == want("n_257")[1]
        hh, hc = vm.rays_host(bp, origin, dims, rays[:0], coarse_ptr=c)
        assert len(hh) == 0 and sum(hc.values()) == 0
    vm.close()


def _raycast_call(vm, bits_ptr, coarse_ptr, origin, dims, W, H, cam, c2w12=None, pose7=None, cell=True, counts=True, **prm):
    import torch
    from stereo_vo_amd import api
    before, stats = TA._frozen(vm)
    dt, dp, dg = _guarded(W * H, torch.int16, SENT16)
    ct, cp, cg = _guarded(W * H, torch.int32, SENT32)
    nt, np_, ng = _guarded(7, torch.int64, SENT)
    torch.cuda.synchronize()
    vm.raycast(bits_ptr, origin, dims, W, H, api.CameraInfo(cam[0], cam[1], cam[2], 0, 0, 0, 0, cam[3]), c2w12=c2w12, pose7=pose7, coarse_ptr=coarse_ptr, disp_ptr=dp,
               cell_ptr=cp if cell else None, counts_ptr=np_ if counts else None, **prm)
    vm.ctx.sync()
    disp = _unguard(dt, dg, SENT16).view(np.int16).reshape(H, W)
    cells = _unguard(ct, cg, SENT32).view(np.uint32).reshape(H, W) if cell else None
    got = _unguard(nt, ng, SENT).view(np.uint64).tolist() if counts else None
    if not cell:
        assert (ct.cpu().numpy() == SENT32).all()
    if not counts:
        assert (nt.cpu().numpy() == SENT).all()
    after, stats2 = TA._frozen(vm)
    assert all(np.array_equal(before[k], after[k]) for k in before) and stats2 == stats
    return disp, cells, got


@pytest.mark.gpu
def test_the_slab_through_the_map_by_every_entry(ctx):
    """The slab inserted into a map, its occupancy and coarse volume from the device, the camera form by both walks, the optional
    outputs left out, odd image sizes (tiles cut by both edges), and the host convenience around the same camera centre."""
    from stereo_vo_amd import api
    pts, m = slab_table()
    vm = TA._build(ctx, [("insert", pts, m)], SLAB_VS, 0.0, 16)
    words, occ, d, bt, bp = _occupancy_call(vm, SLAB_ORIGIN, SLAB_DIMS, 1)
    assert np.array_equal(words, slab_words()) and occ == [128 * 128, 0]
    coarse, ct, cp = _coarse_call(vm, bp, SLAB_DIMS)
    assert np.array_equal(coarse, R.coarse_np(words, SLAB_DIMS))
    (disp, cell, counts), _ = slab_views()
    c2w = TA.ident(SLAB_CENTRE)
    ctx.profile_select("voxel_rays")
    for c in (None, cp):
        got = _raycast_call(vm, bp, c, SLAB_ORIGIN, SLAB_DIMS, *SLAB_WH, SLAB_CAM, c2w12=c2w)
        assert np.array_equal(got[0], disp) and np.array_equal(got[1], cell) and got[2] == counts, c
        got = _raycast_call(vm, bp, c, SLAB_ORIGIN, SLAB_DIMS, *SLAB_WH, SLAB_CAM, c2w12=c2w, cell=False, counts=False)
        assert np.array_equal(got[0], disp)
        for W, H, ms, mr in ((61, 43, 1, 30.0), (9, 1, 0, 2.5), (1, 9, 3, 30.0)):
            cam = (60.0, (W - 1) / 2.0, H / 2.0 - 12.0, 0.5)
            w = R.raycast(words, SLAB_ORIGIN, SLAB_DIMS, W, H, cam, c2w, mr, ms, SLAB_VS)
            got = _raycast_call(vm, bp, c, SLAB_ORIGIN, SLAB_DIMS, W, H, cam, c2w12=c2w, max_range=mr, min_step=ms)
            assert np.array_equal(got[0], w[0]) and np.array_equal(got[1], w[1]) and got[2] == w[2], (c, W, H)
    assert ctx.profile_read()[1] == 10
    ctx.profile_select(None)
    # the pose7 form: a turned camera; its matrix is the library's own
    pose = [0.9689124217106447, 0.0, 0.24740395925452294, 0.0, 0.02, -0.31, 0.04]
    m12 = TA._m(pose)
    w = R.raycast(words, SLAB_ORIGIN, SLAB_DIMS, *SLAB_WH, SLAB_CAM, m12, 30.0, 1, SLAB_VS)
    got = _raycast_call(vm, bp, cp, SLAB_ORIGIN, SLAB_DIMS, *SLAB_WH, SLAB_CAM, pose7=np.array(pose))
    assert np.array_equal(got[0], w[0]) and np.array_equal(got[1], w[1]) and got[2] == w[2] and w[2][6] > 500
    # the host convenience: the volume around the camera centre
    cam = api.CameraInfo(SLAB_CAM[0], SLAB_CAM[1], SLAB_CAM[2], 0, 0, 0, 0, SLAB_CAM[3])
    hd, hc, hn = vm.raycast_host(*SLAB_WH, cam, c2w12=c2w, dims=SLAB_DIMS)
    origin = R.origin_of(SLAB_CENTRE, SLAB_VS, SLAB_DIMS)
    assert hn["origin"] == origin
    w = R.raycast(L.occupancy_np(d, origin, SLAB_DIMS, 1)[0], origin, SLAB_DIMS, *SLAB_WH, SLAB_CAM, c2w, 30.0, 1, SLAB_VS)
    assert np.array_equal(hd, w[0]) and np.array_equal(hc, w[1]) and [hn[k] for k in api.RAYCAST_COUNTS] == w[2]
    vm.close()


CORNER_WH, CORNER_CAM, CORNER_DIMS = (80, 40), (60.0, 40.0, 20.0, 0.5), (256, 64, 256)


@pytest.mark.gpu
@pytest.mark.parametrize("vs,lg", TA.SIZES)
def test_corner_scene_seen_from_its_own_pose(ctx, vs, lg):
    vm = TA._build(ctx, [("insert", TN.corner(10), TA._m(TA.TRUTH))], vs, 0.0, lg)
    m12 = TA._m(TA.TRUTH)
    origin = R.origin_of((m12[3], m12[7], m12[11]), vs, CORNER_DIMS)
    words, occ, d, bt, bp = _occupancy_call(vm, origin, CORNER_DIMS, 1)
    coarse, ct, cp = _coarse_call(vm, bp, CORNER_DIMS)
    assert np.array_equal(coarse, R.coarse_np(words, CORNER_DIMS)) and occ[0] == int(np.unpackbits(words.view(np.uint8)).sum()) > 100
    w = R.raycast(words, origin, CORNER_DIMS, *CORNER_WH, CORNER_CAM, m12, 30.0, 1, vs)
    print("corner", vs, "counts", w[2])
    assert w[2][6] > 1000  # the walls are seen
    for c in (None, cp):
        got = _raycast_call(vm, bp, c, origin, CORNER_DIMS, *CORNER_WH, CORNER_CAM, pose7=np.array(TA.TRUTH))
        assert np.array_equal(got[0], w[0]) and np.array_equal(got[1], w[1]) and got[2] == w[2], c
    # the same pixels as records: narrowed to f32 they are other rays, restated as such
    rows = []
    for y in range(0, CORNER_WH[1], 3):
        for x in range(0, CORNER_WH[0], 3):
            o, dd = R.pixel_ray([float(v) for v in m12], CORNER_CAM, x, y)
            rows.append((*o, 30.0, *dd))
    rays = R.make_rays(rows)
    wh, wc = R.rays(words, origin, CORNER_DIMS, rays, 1, vs)
    for c in (None, cp):
        hits, counts = _rays_call(vm, bp, c, origin, CORNER_DIMS, rays, 1)
        _assert_hits(hits, wh, (vs, c))
        assert counts == wc and wc[0] > 50
    vm.close()


@pytest.mark.gpu
def test_bad_arguments_launch_nothing_and_leave_the_map_usable(ctx):
    import torch
    from stereo_vo_amd import api
    lib = ctx.L
    pts, m = slab_table()
    vm = TA._build(ctx, [("insert", pts[:500], m)], SLAB_VS, 0.0, 12)
    dims = (64, 8, 8)
    bt, bp, bg = _guarded(R.occupancy_words(dims), torch.int64, SENT)
    ct, cp, cg = _guarded(R.coarse_words(dims), torch.int64, SENT)
    ht, hp, hg = _guarded(4 * 5, torch.int32, SENT32)
    nt, np_, ng = _guarded(7, torch.int64, SENT)
    dt, dp, dg = _guarded(64 * 48, torch.int16, SENT16)
    lt, lp, lg = _guarded(64 * 48, torch.int32, SENT32)
    rt, rp, rg = _guarded(8 * 5, torch.int32, SENT32)
    torch.cuda.synchronize()
    I3 = lambda *v: (C.c_int * 3)(*v)
    o3, d3 = I3(0, 0, 0), I3(*dims)
    cam, prm = api.CameraInfo(60.0, 31.5, 23.5, 0, 0, 0, 0, 0.5), api.voxel_raycast_default_params()
    mp = np.ascontiguousarray(TA.ident()).ctypes.data_as(C.c_void_p)
    host = np.zeros(64 * 48, np.int16)

    def P(**kw):
        p = api.VoxelRaycastParams.from_buffer_copy(prm)
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)

    def CAM(**kw):
        c = api.CameraInfo.from_buffer_copy(cam)
        for k, v in kw.items():
            setattr(c, k, v)
        return C.byref(c)

    co = lambda b=None, d=d3, c=None: lib.svo_voxel_occupancy_coarse_dev(vm.h, bp if b is None else b, d, cp if c is None else c)
    ry = lambda b=None, c=None, o=o3, d=d3, r=None, n=5, ms=1, h=None, k=None: lib.svo_voxel_occupancy_rays_dev(
        vm.h, bp if b is None else b, cp if c is None else c, o, d, rp if r is None else r, n, ms, hp if h is None else h, np_ if k is None else k)
    rc = lambda b=None, c=None, o=o3, d=d3, W=64, H=48, cm=C.byref(cam), mm=mp, p=C.byref(prm), dd=None, l=None, k=None: lib.svo_voxel_occupancy_raycast_dev(
        vm.h, bp if b is None else b, cp if c is None else c, o, d, W, H, cm, mm, p, dp if dd is None else dd, lp if l is None else l, np_ if k is None else k)
    hc = lambda mc=1, d=d3, W=64, H=48, cm=C.byref(cam), mm=mp, p=C.byref(prm), dd=host.ctypes.data_as(C.c_void_p): lib.svo_voxel_map_raycast(
        vm.h, mc, d, W, H, cm, mm, p, dd, None, None, None)
    far = np.ascontiguousarray(TA.ident((3.0e5, 0.0, 0.0))).ctypes.data_as(C.c_void_p)      # 3,000,000 voxels out: beyond 2^21
    edge = np.ascontiguousarray(TA.ident((1.04857e5, 0.0, 0.0))).ctypes.data_as(C.c_void_p)  # 1,048,570 voxels out: the volume's end passes 2^20
    calls = [(lambda: co(d=None), "null dims"), (lambda: co(d=I3(96, 1, 1)), "multiple of 64"), (lambda: co(b=0), "null bits"), (lambda: co(b=bp + 4), "8-byte"),
             (lambda: co(c=0), "null coarse"), (lambda: co(c=cp + 4), "coarse must be 8-byte"), (lambda: co(b=0, c=0), "null bits"),
             (lambda: ry(n=-1), "n must not"), (lambda: ry(n=(1 << 20) + 1), "2^20"), (lambda: ry(ms=-1), "min_step"), (lambda: ry(ms=256), "min_step"),
             (lambda: ry(o=None), "null origin"), (lambda: ry(o=I3(0, 1 << 20, 0)), "origin outside"), (lambda: ry(d=None), "null dims"),
             (lambda: ry(d=I3(64, 0, 1)), "dims outside"), (lambda: ry(d=I3(2048, 1024, 1024)), "2^30"), (lambda: ry(b=0), "null bits"), (lambda: ry(b=bp + 4), "bits must be 8-byte"),
             (lambda: ry(c=cp + 4), "coarse must be 8-byte"), (lambda: ry(h=0), "null hits"), (lambda: ry(h=hp + 8), "hits must be 16-byte"),
             (lambda: ry(k=np_ + 4), "counts must be 8-byte"), (lambda: ry(r=0), "null rays"), (lambda: ry(r=rp + 8), "rays must be 16-byte"),
             (lambda: ry(n=-1, ms=256), "n must not"), (lambda: ry(ms=256, o=None), "min_step"), (lambda: ry(c=cp + 4, h=0), "coarse must be"),
             (lambda: lib.svo_voxel_occupancy_rays(vm.h, bp, None, o3, d3, None, 5, 1, host.ctypes.data_as(C.c_void_p), None), "null rays"),
             (lambda: rc(cm=None), "null cam"), (lambda: rc(mm=None), "null c2w12"), (lambda: rc(p=None), "null params"), (lambda: rc(p=P(max_range=-1.0)), "max_range"),
             (lambda: rc(p=P(max_range=float("nan"))), "max_range"), (lambda: rc(p=P(max_range=float("inf"))), "max_range"), (lambda: rc(p=P(min_step=256)), "min_step"),
             (lambda: rc(W=0), "width"), (lambda: rc(W=1281), "width"), (lambda: rc(H=721), "height"), (lambda: rc(cm=CAM(focal=0.0)), "focal"),
             (lambda: rc(cm=CAM(baseline=float("nan"))), "baseline"), (lambda: rc(o=None), "null origin"), (lambda: rc(d=I3(32, 1, 1)), "multiple of 64"),
             (lambda: rc(b=0), "null bits"), (lambda: rc(c=cp + 4), "coarse must be"), (lambda: rc(dd=0), "null disp16"), (lambda: rc(dd=dp + 1), "2-byte"),
             (lambda: rc(l=lp + 2), "cell must be 4-byte"), (lambda: rc(k=np_ + 4), "counts must be 8-byte"), (lambda: rc(p=P(min_step=256), W=0), "min_step"),
             (lambda: lib.svo_voxel_occupancy_raycast_pose7_dev(vm.h, bp, cp, o3, d3, 64, 48, C.byref(cam), None, C.byref(prm), dp, lp, np_), "null pose7"),
             (lambda: hc(mc=0), "min_count"), (lambda: hc(cm=None), "null cam"), (lambda: hc(W=0), "width"), (lambda: hc(d=None), "null dims"),
             (lambda: hc(dd=None), "null disp16"), (lambda: hc(mm=far), "outside the key range"), (lambda: hc(mm=edge), "leaves the key range")]
    assert len(calls) >= 50
    before, stats = TA._frozen(vm)
    for tag in ("voxel_rays", "voxel_coarse", "voxel_occupancy"):
        ctx.profile_select(tag)
        for call, word in calls:
            assert call() == -1 and word in lib.svo_last_error(ctx.h).decode(), (word, lib.svo_last_error(ctx.h).decode())
        assert ctx.profile_read()[1] == 0
        ctx.profile_select(None)
    ctx.sync()
    for tt, s in ((bt, SENT), (ct, SENT), (ht, SENT32), (nt, SENT), (dt, SENT16), (lt, SENT32), (rt, SENT32)):
        assert (tt.cpu().numpy() == s).all()
    assert not host.any()
    after, stats2 = TA._frozen(vm)
    assert all(np.array_equal(before[k], after[k]) for k in before) and stats2 == stats
    # the context and the map work
    words, occ, d, bt2, bp2 = _occupancy_call(vm, SLAB_ORIGIN, SLAB_DIMS, 1)
    assert occ == [500, 0] and np.array_equal(_coarse_call(vm, bp2, SLAB_DIMS)[0], R.coarse_np(words, SLAB_DIMS))
    vm.close()
