"""Free-space carving and the copy of the live voxels (include/svo.h, "Free-space carving") against their restatement
tests/voxel_carve_ref.py, with ==.

CPU: the restatement's two routes agree on every scene used below; svo_pose7_to_world_to_cam; the refusals that need no context;
each deliberate misreading of the contract changes a carve of the main scene.
GPU: the downloaded table sorted by key (carved slots keep their key and hold four zero words), the three counts and the extraction
sorted by record bytes equal the restatement.  Two facts about the main scene are CONDITIONS, asserted on the restatement before
any comparison: no voxel outside the box is carved by view B, and view A carves nothing of its own map at the default parameters.

The main scene (160 x 80, f = 120, B = 0.5): wall at 8 m, panel at 5 m for x < -1, box at 3 m; view A at the origin with the box,
view B at (0.35, 0.1, 0) without it, with a 4 x 10 FILTERED patch over the box's right edge and one pixel at 0.  On the restatement
(margin16 8): 0.05 m 10,903 voxels, 360 of the box, 353 / 347 / 338 carved at radius 0 / 1 / 2, 111 of the 347 at keep_count 4;
0.1 m 5,239 / 100, 98 / 97 / 95 carved, none at keep_count 4; 0.25 m 1,376 / 32, 32 / 30 / 30 carved.  View A on its own map: 0 at
radius 0 with margin16 3 and at the defaults; 10,755 / 4,718 / 460 at margin16 0.
Misreadings, voxels whose fate changes: the centre pixel instead of the window maximum 1,107 (0.05 m, radius 1, margin16 2); <=
instead of < 187 (0.25 m, radius 0, margin16 0: a voxel of points at exactly 8 m has dv16 = 120 = the map's value); trunc(u) 6,
the voxel centre 3, an invalid pixel read as 0 13 (0.05 m, defaults); count > keep_count 125 (0.05 m, keep_count 4).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import voxel_carve_ref as R
import voxel_ref as V
from test_voxel_map import IDENT, _fits, _insert, _map

SIZES = ((0.05, 15), (0.1, 14), (0.25, 14))  # voxel size, table log2
A2W, W2A, B2W, W2B = (R.shift(c, w) for c in (R.VIEW_A, R.VIEW_B) for w in (True, False))
POSE_B = np.array([1.0, 0, 0, 0, -R.VIEW_B[0], -R.VIEW_B[1], -R.VIEW_B[2]])  # X_cam = X_world - centre
# bounds on voxel faces of the 0.25 m grid, the doubles just beside them, and half-open ones
BOXES = (None, (-1.0, -2.0, 2.9, 1.0, 2.0, 8.2), (np.nextafter(-1.0, -2.0), -2.0, 2.9, np.nextafter(1.0, 0.0), 2.0, 8.2),
         (-np.inf, -np.inf, 0.0, np.inf, 0.1, 6.0))
MISREADINGS = {  # variant -> (voxel size, radius, margin16, keep_count) of a carve of A's map with view B
    "centre": (0.05, 1, 2, 0), "le": (0.25, 0, 0, 0), "trunc": (0.05, 1, 8, 0), "voxel_centre": (0.05, 1, 8, 0),
    "invalid_as_zero": (0.05, 1, 8, 0), "keep_gt": (0.05, 1, 8, 4)}


@functools.lru_cache(maxsize=None)
def scene():
    pts, da, is_box, db = R.main_scene()
    for a in (pts, da, is_box, db):
        a.setflags(write=False)
    return pts, da, is_box, db


@functools.lru_cache(maxsize=None)
def table_a(vs):
    return V.insert_np(scene()[0], A2W, vs)


@functools.lru_cache(maxsize=None)
def box_keys(vs):
    pts, _, is_box, _ = scene()
    return frozenset(V.insert_np(pts[is_box], A2W, vs).keys.tolist())


@functools.lru_cache(maxsize=None)
def carved_by_b(vs, radius, margin16=8, keep_count=0):
    return R.carve_np(table_a(vs), scene()[3], R.CAM, W2B, vs, radius, margin16, keep_count)


@functools.lru_cache(maxsize=None)
def conditions():
    """The two facts the comparisons below stand on, on the restatement."""
    for vs, _ in SIZES:
        for radius in (0, 1, 2):
            after, _ = carved_by_b(vs, radius)
            assert not (R.carved_set(table_a(vs), after) - box_keys(vs)), (vs, radius)  # no non-box voxel is carved
        _, counts = R.carve_np(table_a(vs), scene()[1], R.CAM, W2A, vs)  # the own view, default parameters
        assert counts[1] > 1000 and counts[2] == 0, (vs, counts)
    return True


def _cam():
    from stereo_vo_amd import api
    f, cx, cy, b = R.CAM
    return api.CameraInfo(f, cx, cy, 0, 0, 0, 0, b)


# ------------------------------------------------------------------------------------------------ constructed single voxels
def _const_map(value, **pixels):
    d = np.full((R.H, R.W), value, np.int16)
    for k, v in pixels.items():
        y, x = (int(s) for s in k[1:].split("_"))
        d[y, x] = v
    return d


def _unit(z_scale=1.0, tz=0.0):
    return np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, z_scale, tz], np.float64)


@functools.lru_cache(maxsize=None)
def singles():
    """name -> (records, disp16, cam 4-tuple, world->camera, radius, margin16, keep_count, expected (n_tested, n_carved)).  Voxel
    size 0.25 under identity: a point at (0.25, 0, 4) is a voxel whose mean is exactly that, dv16 = 16 * 60 / 4 = 240, u = 120 *
    0.25 / 4 + cx = 7.5 + cx, v = cy."""
    f, cx, cy, b = R.CAM
    one = lambda x, y, z: V.records(np.float32([x]), np.float32([y]), np.float32([z]), np.uint32([0x40000000]))
    P = one(0.25, 0.0, 4.0)
    out = {
        "margin_not_below": (P, _const_map(232), R.CAM, _unit(), 0, 8, 0, (1, 0)),      # 232 + 8 < 240 is false
        "margin_below": (P, _const_map(231), R.CAM, _unit(), 0, 8, 0, (1, 1)),
        "u_87_5_rounds_to_88": (P, _const_map(232, p40_88=231), R.CAM, _unit(), 0, 8, 0, (1, 1)),
        "u_87_5_is_not_87": (P, _const_map(232, p40_87=231), R.CAM, _unit(), 0, 8, 0, (1, 0)),
        "v_rounds_half_up": (one(0.25, 0.25, 4.0), _const_map(232, p48_88=231), (f, cx, cy + 0.0, b), _unit(), 0, 8, 0, (1, 1)),
        "c2_zero": (P, _const_map(100), R.CAM, _unit(tz=-4.0), 0, 8, 0, (0, 0)),
        "c2_negative": (P, _const_map(100), R.CAM, _unit(tz=-5.0), 0, 8, 0, (0, 0)),
        # c_2 = 4e-310: u = 30 / c_2 overflows for the first voxel (not tested); for the second c_0 = 0, u = cx, dv16 = infinity
        "c2_tiny": (np.concatenate([P, one(0.0, 0.0, 4.0)]), _const_map(100), R.CAM, _unit(z_scale=1e-310), 0, 8, 0, (1, 1)),
        "keep_count_reached": (np.concatenate([P, P, P]), _const_map(100), R.CAM, _unit(), 0, 8, 3, (1, 0)),
        "keep_count_not_reached": (np.concatenate([P, P]), _const_map(100), R.CAM, _unit(), 0, 8, 3, (1, 1)),
    }
    for radius in (0, 1, 3):  # px = floor(cx' + 7.5 + 0.5) at the bounds of the tested range and one outside each
        for name, px, tested in (("at_low", radius, 1), ("below_low", radius - 1, 0), ("at_high", R.W - 1 - radius, 1),
                                 ("above_high", R.W - radius, 0)):
            out[f"px_{name}_r{radius}"] = (P, _const_map(100), (f, px - 7.5, cy, b), _unit(), radius, 8, 0, (tested, tested))
        out[f"py_above_high_r{radius}"] = (P, _const_map(100), (f, cx, float(R.H - radius), b), _unit(), radius, 8, 0, (0, 0))
        out[f"py_at_high_r{radius}"] = (P, _const_map(100), (f, cx, float(R.H - 1 - radius), b), _unit(), radius, 8, 0, (1, 1))
    # u = radius - 0.5 exactly rounds up into the range; the next double below it does not
    out["px_half_below_low"] = (P, _const_map(100), (f, 1 - 8.0, cy, b), _unit(), 1, 8, 0, (1, 1))
    out["px_just_under_half"] = (P, _const_map(100), (f, np.nextafter(-7.0, -8.0), cy, b), _unit(), 1, 8, 0, (0, 0))
    for name, bad in (("filtered", R.FILTERED), ("zero", 0), ("negative", -5)):
        out[f"window_holds_{name}"] = (P, _const_map(100, p41_89=bad), R.CAM, _unit(), 1, 8, 0, (1, 0))
        out[f"window_misses_{name}"] = (P, _const_map(100, p41_89=bad), R.CAM, _unit(), 0, 8, 0, (1, 1))
    out["window_maximum_decides"] = (P, _const_map(100, p39_87=232), R.CAM, _unit(), 1, 8, 0, (1, 0))
    return out


def _single_want(name):
    p, disp, cam, m, radius, margin, keep, expect = singles()[name]
    t = V.insert_np(p, IDENT, 0.25)
    after, counts = R.carve_np(t, disp, cam, m, 0.25, radius, margin, keep)
    return t, after, counts


# ===================================================================================================== CPU
def test_the_two_routes_of_the_restatement_agree_on_every_scene():
    pts, da, _, db = scene()
    for vs, _ in SIZES:
        t = table_a(vs)
        for disp, m in ((db, W2B), (da, W2A)):
            for radius, margin, keep in ((0, 8, 0), (1, 8, 0), (2, 8, 0), (1, 8, 4), (0, 0, 0), (0, 3, 0), (1, 2, 4)):
                a, ca = R.carve_np(t, disp, R.CAM, m, vs, radius, margin, keep)
                b, cb = R.carve_py(t, disp, R.CAM, m, vs, radius, margin, keep)
                assert V.same(a, b) and ca == cb, (vs, radius, margin, keep)
                assert ca[0] == len(t.keys) and ca[2] == len(R.carved_set(t, a))
        # a second carve finds the carved slots dead; insert - carve - insert restarts them
        a, ca = carved_by_b(vs, 1)
        b, cb = R.carve_py(a, db, R.CAM, W2B, vs, 1, 8, 0)
        assert cb == R.carve_np(a, db, R.CAM, W2B, vs, 1, 8, 0)[1] == (ca[0] - ca[2], ca[1] - ca[2], 0) and V.same(a, b)
    for name, (p, disp, cam, m, radius, margin, keep, expect) in singles().items():
        t, a, ca = _single_want(name)
        b, cb = R.carve_py(t, disp, cam, m, 0.25, radius, margin, keep)
        assert V.same(a, b) and ca == cb, name
        assert ca[1:] == expect and ca[0] == len(t.keys), (name, ca)  # and both give what the scene was built to give


def test_the_main_scene_is_what_the_comparisons_need():
    assert conditions()
    assert [len(table_a(vs).keys) for vs, _ in SIZES] == [10903, 5239, 1376]
    assert [len(box_keys(vs)) for vs, _ in SIZES] == [360, 100, 32]
    got = [[carved_by_b(vs, radius)[1][2] for radius in (0, 1, 2)] for vs, _ in SIZES]
    assert got == [[353, 347, 338], [98, 97, 95], [32, 30, 30]], got
    assert carved_by_b(0.05, 1, 8, 4)[1][2] == 111 and carved_by_b(0.1, 1, 8, 4)[1][2] == 0
    for vs, _ in SIZES:  # the own view: nothing at radius 0 from margin16 3 on, a lot at margin16 0
        assert R.carve_np(table_a(vs), scene()[1], R.CAM, W2A, vs, 0, 3, 0)[1][2] == 0
        assert R.carve_np(table_a(vs), scene()[1], R.CAM, W2A, vs, 0, 0, 0)[1][2] > 400
    db = scene()[3]
    assert int((db == R.FILTERED).sum()) == 40 and int((db == 0).sum()) == 1 and int((db <= 0).sum()) == 41


def test_every_misreading_of_the_contract_changes_the_carved_set():
    db = scene()[3]
    got = {}
    for variant, (vs, radius, margin, keep) in MISREADINGS.items():
        t = table_a(vs)
        right, _ = R.carve_np(t, db, R.CAM, W2B, vs, radius, margin, keep)
        wrong, _ = R.carve_np(t, db, R.CAM, W2B, vs, radius, margin, keep, variant=variant)
        got[variant] = len(R.carved_set(t, right) ^ R.carved_set(t, wrong))
        assert got[variant] > 0, variant
    assert set(got) == set(R.VARIANTS)
    assert got == {"centre": 1107, "le": 187, "trunc": 6, "voxel_centre": 3, "invalid_as_zero": 13, "keep_gt": 125}, got


def test_the_copy_restated():
    t = table_a(0.25)
    assert V.same(V.merge(R.empty_table(), R.copy_live(t, 0.25)), t._replace(n_rejected=0))
    on, beside = R.copy_live(t, 0.25, 1, BOXES[1]), R.copy_live(t, 0.25, 1, BOXES[2])
    kx = lambda c: sorted(set(((c.keys & np.uint64(0x1FFFFF)).astype(np.int64) - (1 << 20)).tolist()))
    assert kx(on) == list(range(-4, 5)) and kx(beside) == list(range(-5, 4))  # a bound on a face belongs to the voxel above it
    assert 0 < len(R.copy_live(t, 0.25, 3).keys) < len(t.keys)


def test_pose7_to_world_to_cam_on_the_cpu():
    from stereo_vo_amd import api
    rng = np.random.default_rng(5)
    for scale in (1.0, 0.37, 5.0):
        q = rng.normal(size=4)
        pose = np.concatenate([scale * q / np.linalg.norm(q), rng.normal(size=3) * 4])
        m = api.pose7_to_world_to_cam(pose)
        want = R.world_to_cam(pose)
        assert np.allclose(m, want, rtol=0, atol=1e-14), (m - want)
        back = api.pose7_to_cam_to_world(pose)
        prod = np.vstack([m, [0, 0, 0, 1]]) @ np.vstack([back, [0, 0, 0, 1]])
        assert np.allclose(prod, np.eye(4), rtol=0, atol=1e-12), prod - np.eye(4)
    assert np.array_equal(api.pose7_to_world_to_cam([2, 0, 0, 0, 1, -2, 3]), np.hstack([np.eye(3), [[1], [-2], [3]]]))
    assert np.array_equal(api.pose7_to_world_to_cam(POSE_B).reshape(12), W2B)


def test_pure_entries_and_refusals_without_a_context():
    from stereo_vo_amd import api
    L = api.lib()
    d = api.voxel_carve_default_params()
    assert (d.radius, d.margin16, d.keep_count) == (1, 8, 0)
    assert L.svo_voxel_carve_default_params(None) == -1
    buf = (C.c_double * 12)()
    assert L.svo_pose7_to_world_to_cam(None, buf) == -1 and L.svo_pose7_to_world_to_cam(buf, None) == -1
    cam = _cam()
    # a null map is refused by every entry
    assert L.svo_voxel_map_carve_dev(None, buf, 16, 16, C.byref(cam), buf, C.byref(d), None) == -1
    assert L.svo_voxel_map_carve_pose7_dev(None, buf, 16, 16, C.byref(cam), buf, C.byref(d), None) == -1
    assert L.svo_voxel_map_carve(None, buf, 16, 16, C.byref(cam), buf, C.byref(d), None) == -1
    assert L.svo_voxel_map_copy_live_dev(None, None, 1, None) == -1
    assert L.svo_pipeline_keyframe_disparity(None, 0, buf) == -1 and L.svo_pipeline_group_keyframe_disparity(None, 0, buf) == -1
    assert L.svo_pipeline_copy_keyframe_disparity(None, 0, buf) == -1 and L.svo_pipeline_group_copy_keyframe_disparity(None, 0, buf) == -1


# ===================================================================================================== GPU
def _table_of(vm):
    """The downloaded table sorted by key, carved slots included."""
    d = vm.download()
    occ = d["keys"] != np.uint64(V.EMPTY)
    for k in ("ci", "sx", "sy", "sz"):
        assert not d[k][~occ].any(), k  # an empty slot has no payload
    o = np.argsort(d["keys"][occ])
    return tuple(d[k][occ][o] for k in ("keys", "ci", "sx", "sy", "sz"))


def _assert_table(vm, want, what=""):
    for g, name in zip(_table_of(vm), ("keys", "ci", "sx", "sy", "sz")):
        assert np.array_equal(g, getattr(want, name)), (what, name)


def _assert_extraction(vm, want, vs, what=""):
    for min_count in (1, 3):
        pts, n_total = vm.extract(min_count)
        ref = V.extract(want, vs, min_count)
        assert n_total == len(ref) == len(pts) and np.array_equal(V.sort_records(pts), ref), (what, min_count)


def _carve(vm, disp, cam4, m12, radius, margin, keep, how):
    """One carve by the named entry; the three counts (None for "nocounts")."""
    import torch
    from stereo_vo_amd import api
    cam = api.CameraInfo(cam4[0], cam4[1], cam4[2], 0, 0, 0, 0, cam4[3])
    h, w = disp.shape
    if how == "host":
        c = vm.carve_host(disp, cam, w2c12=m12, radius=radius, margin16=margin, keep_count=keep)
        return c["n_live"], c["n_tested"], c["n_carved"]
    dd = torch.from_numpy(np.array(disp, np.int16)).cuda()
    cnt = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    kw = dict(radius=radius, margin16=margin, keep_count=keep, counts_ptr=None if how == "nocounts" else cnt.data_ptr())
    if how == "pose7":
        assert np.array_equal(np.asarray(m12).reshape(3, 4)[:, :3], np.eye(3))
        vm.carve(dd.data_ptr(), w, h, cam, pose7=np.concatenate([[1.0, 0, 0, 0], np.asarray(m12).reshape(3, 4)[:, 3]]), **kw)
    else:
        vm.carve(dd.data_ptr(), w, h, cam, w2c12=m12, **kw)
    vm.ctx.sync()  # the tensors go out of scope behind this line
    got = tuple(cnt.cpu().tolist())
    if how == "nocounts":
        assert got == (-1, -1, -1)
        return None
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("radius", (0, 1, 2))
@pytest.mark.parametrize("vs,lg", SIZES)
def test_main_scene_carved_by_view_b(ctx, vs, lg, radius):
    assert conditions()
    pts, _, _, db = scene()
    t = table_a(vs)
    _fits(t.keys, lg)
    for keep, how in ((0, "dev"), (4, "pose7"), (4, "host")):
        want, counts = carved_by_b(vs, radius, 8, keep)
        vm = _map(ctx, vs, lg)
        _insert(vm, pts, A2W)
        before, stats = vm.download()["keys"].copy(), vm.stats()
        assert _carve(vm, db, R.CAM, W2B, radius, 8, keep, how) == counts, (keep, how)
        _assert_table(vm, want, (keep, how))
        assert np.array_equal(vm.download()["keys"], before) and vm.stats() == stats  # the keys stay; n_voxels is "slots claimed"
        _assert_extraction(vm, want, vs, (keep, how))
        vm.close()


@pytest.mark.gpu
def test_own_view_carves_nothing_and_a_second_carve_finds_the_slots_dead(ctx):
    assert conditions()
    pts, da, _, db = scene()
    vs, lg = 0.1, 14
    t = table_a(vs)
    vm = _map(ctx, vs, lg)
    _insert(vm, pts, A2W)
    assert _carve(vm, da, R.CAM, W2A, 1, 8, 0, "dev") == R.carve_np(t, da, R.CAM, W2A, vs)[1]
    _assert_table(vm, t)
    want, counts = carved_by_b(vs, 1)
    assert _carve(vm, db, R.CAM, W2B, 1, 8, 0, "nocounts") is None
    _assert_table(vm, want)
    again, c2 = R.carve_np(want, db, R.CAM, W2B, vs)
    assert c2 == (counts[0] - counts[2], counts[1] - counts[2], 0)
    assert _carve(vm, db, R.CAM, W2B, 1, 8, 0, "dev") == c2
    _assert_table(vm, again)
    vm.close()


@pytest.mark.gpu
def test_insert_carve_insert(ctx):
    assert conditions()
    pts, _, _, db = scene()
    vs, lg = 0.05, 15
    t = table_a(vs)
    carved, counts = carved_by_b(vs, 1)
    want = V.merge(carved, t)  # the carved voxels start again from the second cloud alone
    assert counts[2] > 300 and V.changed_voxels(want, V.merge(t, t)) == counts[2]
    _fits(t.keys, lg)
    vm = _map(ctx, vs, lg)
    _insert(vm, pts, A2W)
    assert _carve(vm, db, R.CAM, W2B, 1, 8, 0, "dev") == counts
    _insert(vm, pts, A2W)
    _assert_table(vm, want)
    assert vm.stats() == {"n_voxels": len(t.keys), "n_inserted": 2 * t.n_inserted, "n_rejected": 2 * t.n_rejected, "n_dropped": 0}
    _assert_extraction(vm, want, vs)
    vm.close()


@pytest.mark.gpu
def test_constructed_single_voxels_in_a_table_smaller_than_one_tile(ctx):
    vm = _map(ctx, 0.25, 8)  # 256 slots: one workgroup walks 2,048
    for i, (name, (p, disp, cam, m, radius, margin, keep, expect)) in enumerate(sorted(singles().items())):
        t, want, counts = _single_want(name)
        assert counts[1:] == expect, name
        vm.clear()
        _insert(vm, p, IDENT)
        assert _carve(vm, disp, cam, m, radius, margin, keep, ("dev", "host")[i % 2]) == counts, name
        _assert_table(vm, want, name)
        pts, n_total = vm.extract(1)
        assert n_total == counts[0] - counts[2] and np.array_equal(V.sort_records(pts), V.extract(want, 0.25, 1)), name
    vm.close()


def _copied(ctx, src, dst_lg, vs, min_count, box, dst_before=None):
    """dst after src.copy_live_to(dst): (VoxelMap, its stats)."""
    dst = _map(ctx, vs, dst_lg)
    if dst_before is not None:
        _insert(dst, *dst_before)
    src.copy_live_to(dst, min_count, box)
    return dst, dst.stats()


@pytest.mark.gpu
@pytest.mark.parametrize("vs,lg", ((0.1, 14), (0.25, 11)))
def test_copy_of_the_main_scene(ctx, vs, lg):
    pts = scene()[0]
    t = table_a(vs)
    _fits(t.keys, lg)
    src = _map(ctx, vs, lg)
    _insert(src, pts, A2W)
    sets = []
    for min_count in (1, 3):
        for box in BOXES:
            moved = R.copy_live(t, vs, min_count, box)
            want = V.merge(R.empty_table(), moved)
            assert 0 < len(want.keys) and (len(want.keys) == len(t.keys)) == (min_count == 1 and box is None)
            _fits(want.keys, lg)
            dst, stats = _copied(ctx, src, lg, vs, min_count, box)
            _assert_table(dst, want, (min_count, box))
            assert stats == {"n_voxels": len(want.keys), "n_inserted": moved.n_inserted, "n_rejected": 0, "n_dropped": 0}
            _assert_extraction(dst, want, vs)
            dst.close()
            sets.append(len(want.keys))
    assert vs != 0.25 or sets[1] != sets[2]  # the bound on a voxel face and the one beside it select different voxels
    _assert_table(src, t)  # the source is only read
    src.close()


@pytest.mark.gpu
def test_copy_after_a_carve_reclaims_the_slots_and_copy_into_a_filled_map_merges(ctx):
    assert conditions()
    pts, _, _, db = scene()
    vs, lg = 0.05, 15
    t = table_a(vs)
    carved, counts = carved_by_b(vs, 1)
    src = _map(ctx, vs, lg)
    _insert(src, pts, A2W)
    assert _carve(src, db, R.CAM, W2B, 1, 8, 0, "dev") == counts
    moved = R.copy_live(carved, vs)
    want = V.merge(R.empty_table(), moved)
    assert len(want.keys) == len(t.keys) - counts[2]
    dst, stats = _copied(ctx, src, lg, vs, 1, None)
    _assert_table(dst, want)
    got = _table_of(dst)
    assert ((got[1] >> np.uint64(40)) >= np.uint64(1)).all()  # no zero-count slot
    d = dst.download()["keys"]
    assert int((d != np.uint64(V.EMPTY)).sum()) == int(V.occupied(want.keys, lg).sum()) < int(V.occupied(t.keys, lg).sum())
    assert stats == {"n_voxels": len(want.keys), "n_inserted": moved.n_inserted, "n_rejected": 0, "n_dropped": 0}
    dst.close()
    # into a map that already holds view B's cloud: a merge
    clean_b, _ = R.render(R.VIEW_B, False, 21)
    pts_b = R.cloud(clean_b, 23)
    tb = V.insert_np(pts_b, B2W, vs)
    want = V.merge(tb, moved)
    assert len(want.keys) < len(tb.keys) + len(moved.keys)  # the views overlap
    _fits(want.keys, lg)
    dst, stats = _copied(ctx, src, lg, vs, 1, None, dst_before=(pts_b, B2W))
    _assert_table(dst, want)
    assert stats == {"n_voxels": len(want.keys), "n_inserted": tb.n_inserted + moved.n_inserted, "n_rejected": tb.n_rejected, "n_dropped": 0}
    _assert_extraction(dst, want, vs)
    dst.close()
    src.close()


@pytest.mark.gpu
def test_copy_into_a_map_too_small_keeps_the_overflow_invariants(ctx):
    pts = scene()[0]
    vs = 0.15
    t = V.insert_np(pts, A2W, vs)
    _fits(t.keys, 14)
    assert len(t.keys) < 1 << 12 and V.longest_run(V.occupied(t.keys, 12)) >= V.MAX_PROBES  # 3,355 voxels, a run of 143
    src = _map(ctx, vs, 14)
    _insert(src, pts, A2W)
    dst, s = _copied(ctx, src, 12, vs, 1, None)
    keys, ci, sx, sy, sz = _table_of(dst)
    true = {int(k): i for i, k in enumerate(t.keys.tolist())}
    assert len(set(keys.tolist())) == len(keys)
    idx = np.array([true.get(int(k), -1) for k in keys.tolist()])
    assert (idx >= 0).all()  # every stored key is a key of the source
    for g, name in ((ci, "ci"), (sx, "sx"), (sy, "sy"), (sz, "sz")):
        assert (g <= getattr(t, name)[idx]).all(), name  # stored words <= the true ones
    count = ci >> np.uint64(40)
    assert s["n_voxels"] == len(keys) and s["n_inserted"] == int(count.sum()) and s["n_rejected"] == 0
    assert s["n_inserted"] + s["n_dropped"] == t.n_inserted and s["n_dropped"] > 0
    dst.close()
    _assert_table(src, t)
    src.close()


@pytest.mark.gpu
def test_bad_arguments_launch_nothing_and_leave_both_maps_usable(ctx):
    import torch
    from stereo_vo_amd import api
    L = ctx.L
    pts, _, _, db = scene()
    vs, lg = 0.25, 11
    t = table_a(vs)
    vm, other, coarse = _map(ctx, vs, lg), _map(ctx, vs, lg), _map(ctx, 0.5, lg)
    _insert(vm, pts, A2W)
    dd = torch.from_numpy(np.array(db, np.int16)).cuda()
    cnt = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    cam, m, q = _cam(), np.ascontiguousarray(W2B), np.ascontiguousarray(POSE_B)
    mp, qp = m.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p)
    P = api.VoxelCarveParams
    dev = lambda **k: L.svo_voxel_map_carve_dev(vm.h, k.get("disp", dd.data_ptr()), k.get("w", R.W), k.get("h", R.H), k.get("cam", C.byref(cam)),
                                                k.get("m", mp), k.get("prm", C.byref(k.get("P", P(1, 8, 0)))), cnt.data_ptr())
    zero_f, zero_b = api.CameraInfo(0, 80, 40, 0, 0, 0, 0, 0.5), api.CameraInfo(120, 80, 40, 0, 0, 0, 0, 0)
    ctx.profile_select("voxel_carve")
    calls = [(lambda: dev(disp=None), "disp16"), (lambda: dev(cam=None), "cam"), (lambda: dev(m=None), "w2c12"), (lambda: dev(prm=None), "params"),
             (lambda: dev(P=P(-1, 8, 0)), "radius"), (lambda: dev(P=P(4, 8, 0)), "radius"),
             (lambda: dev(P=P(1, -1, 0)), "margin16"), (lambda: dev(P=P(1, 32768, 0)), "margin16"), (lambda: dev(P=P(1, 8, -1)), "keep_count"),
             (lambda: dev(w=2), "width"), (lambda: dev(h=2), "height"), (lambda: dev(w=1281), "width"), (lambda: dev(h=721), "height"),
             (lambda: dev(cam=C.byref(zero_f)), "focal"), (lambda: dev(cam=C.byref(zero_b)), "baseline"),
             (lambda: L.svo_voxel_map_carve_pose7_dev(vm.h, dd.data_ptr(), R.W, R.H, C.byref(cam), None, C.byref(P(1, 8, 0)), None), "pose7"),
             (lambda: L.svo_voxel_map_carve(vm.h, None, R.W, R.H, C.byref(cam), mp, C.byref(P(1, 8, 0)), None), "disp16"),
             (lambda: L.svo_voxel_map_carve(vm.h, db.ctypes.data_as(C.c_void_p), R.W, R.H, C.byref(cam), mp, C.byref(P(9, 8, 0)), None), "radius")]
    for call, word in calls:
        assert call() == -1 and word in L.svo_last_error(ctx.h).decode(), word
    assert ctx.profile_read()[1] == 0
    assert dev(w=3, h=3, P=P(1, 8, 0)) == 0  # the smallest map a radius admits is taken
    assert ctx.profile_read()[1] == 1
    ctx.profile_select("voxel_copy")
    nan_box = np.array([0, 0, 0, 1, float("nan"), 1.0])
    calls = [(lambda: L.svo_voxel_map_copy_live_dev(vm.h, vm.h, 1, None), "same map"),
             (lambda: L.svo_voxel_map_copy_live_dev(vm.h, coarse.h, 1, None), "voxel_size"),
             (lambda: L.svo_voxel_map_copy_live_dev(vm.h, other.h, 0, None), "min_count"),
             (lambda: L.svo_voxel_map_copy_live_dev(vm.h, other.h, 1, nan_box.ctypes.data_as(C.c_void_p)), "box6"),
             (lambda: L.svo_voxel_map_copy_live_dev(vm.h, None, 1, None), None), (lambda: L.svo_voxel_map_copy_live_dev(None, other.h, 1, None), None)]
    for call, word in calls:
        assert call() == -1 and (word is None or word in L.svo_last_error(ctx.h).decode()), word
    assert ctx.profile_read()[1] == 0
    ctx.profile_select(None)
    with pytest.raises(ValueError):
        vm.carve(dd.data_ptr(), R.W, R.H, cam)
    with pytest.raises(ValueError):
        vm.carve_host(db, cam, w2c12=m, pose7=q)
    # a second context: its map is refused as the other side of a copy
    import stereo_vo_amd as S
    ctx2 = S.Context(64, 64, max_corners=64)
    foreign = _map(ctx2, vs, 8)
    assert L.svo_voxel_map_copy_live_dev(vm.h, foreign.h, 1, None) == -1 and "context" in L.svo_last_error(ctx2.h).decode()
    foreign.close()
    ctx2.close()
    # nothing was carved or copied except by the 3 x 3 call, whose map (the top left corner of B's) shows the wall only; both maps work
    small, _ = R.carve_np(t, db.ravel()[:9].reshape(3, 3), R.CAM, W2B, vs)
    _assert_table(vm, small)
    assert other.stats() == {"n_voxels": 0, "n_inserted": 0, "n_rejected": 0, "n_dropped": 0}
    want, counts = R.carve_np(small, db, R.CAM, W2B, vs)
    assert _carve(vm, db, R.CAM, W2B, 1, 8, 0, "pose7") == counts
    _assert_table(vm, want)
    vm.copy_live_to(other)
    _assert_table(other, V.merge(R.empty_table(), R.copy_live(want, vs)))
    for m_ in (vm, other, coarse):
        m_.close()
