"""The voxel map's render (include/svo.h, "Voxel map render") against its restatement tests/voxel_render_ref.py, with ==
on the disparity map, the intensity image and the four counts.

CPU: the restatement's two routes agree on every scene used below; the main scene's counts and the facts the comparisons stand on are
asserted on the restatement; each deliberate misreading of the contract changes a render of the main scene; the pure entries and the
refusals that need no context.
GPU: the main scene through the _dev, pose7 and host entries; NULL intensity and NULL counts; record order; render after a carve;
a map never carves itself through its own render; the render as the input of the cloud launch; image sizes that reach the resolve's
tail; the drawing modes; constructed single voxels; bad arguments.

The main scene is tests/voxel_carve_ref.py's (160 x 80, f = 120, B = 0.5; wall at 8 m, panel at 5 m, box at 3 m; view A inserted,
views A at the origin and B at (0.35, 0.1, 0) rendered).  On the restatement at the defaults: 0.05 m 10,903 qualifying, all drawn at
A, 0 FILTERED pixels of 12,800, 10,186 drawn at B; 0.1 m 5,239 / 5,239, 4 FILTERED, 5,011 at B; 0.25 m 1,376 / 1,376, 0 FILTERED, 1,322
at B, radii 2, 3 and 5.  With max_radius 0 every drawn pixel of A is within 2 sixteenths (the scene's noise) of A's measured map.  The
render carves nothing of its own map at radius 0, margin16 1 (both views, all sizes) and 8,165 / 2,134 / 359 voxels (view A) at
margin16 0.
Misreadings, pixels of 12,800 whose disparity or intensity changes: min for max 5,724 (0.05 m, view A); r = floor(h) 3,344 (0.25 m,
A); d16 = floor(dv16) 933 (0.05 m, A); the centre must lie inside the image 163 (0.25 m, view B); intensity left out of the key
2,662 (0.05 m, A); count > min_count 935 (0.05 m, A, min_count 3).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import voxel_carve_ref as R
import voxel_ref as V
import voxel_render_ref as RR
from test_voxel_carve import A2W, POSE_B, SIZES, W2A, W2B, _cam, scene, table_a
from test_voxel_map import IDENT, _fits, _insert, _map

VIEWS = {"A": (W2A, np.array([1.0, 0, 0, 0, 0, 0, 0])), "B": (W2B, POSE_B)}
RADII, MIN_COUNTS = (0, 1, 8), (1, 3)
MISREADINGS = {  # variant -> (voxel size, view, min_count) of a render at max_radius 8, and the pixels it changes
    "min": (0.05, "A", 1, 5724), "r_floor": (0.25, "A", 1, 3344), "d_trunc": (0.05, "A", 1, 933), "centre_inside": (0.25, "B", 1, 163),
    "no_intensity": (0.05, "A", 1, 2662), "count_gt": (0.05, "A", 3, 935)}
# image sizes for the resolve: a tail of 3, 3, 1 pixels behind the groups of four, and a width that is a multiple of 64
SHAPES = ((161, 79), (7, 5), (1, 1), (128, 40))


def _scaled_cam(w, h):
    """The main scene's camera for another image size: the same field of view across the width."""
    f, _, _, b = R.CAM
    return (f * w / R.W, w / 2.0, h / 2.0, b)


@functools.lru_cache(maxsize=None)
def want(vs, view, max_radius=8, min_count=1, shape=None):
    w, h = shape or (R.W, R.H)
    cam = R.CAM if shape is None else _scaled_cam(w, h)
    out = RR.render_np(table_a(vs), w, h, cam, VIEWS[view][0], vs, min_count, max_radius)
    for a in out[:2]:
        a.setflags(write=False)
    return out


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and tuple(a[2]) == tuple(b[2])


# ------------------------------------------------------------------------------------------------ constructed single voxels
def _unit(z_scale=1.0, tz=0.0):
    return np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, z_scale, tz], np.float64)


def _one(x, y, z, inten=0x40, n=1):
    return V.records(np.float32([x] * n), np.float32([y] * n), np.float32([z] * n), np.uint32([inten << 24] * n))


def _below(x):
    return float(np.nextafter(x, 0.0))


@functools.lru_cache(maxsize=None)
def singles():
    """name -> (records, cam 4-tuple, world->camera, min_count, max_radius, expected counts (n_qualifying, n_drawn, n_splat,
    n_pixels), expected drawn voxels as (px, py, r, d16) in table order).  Voxel size 0.25 under identity: a point at (0.25, 0, 4)
    is a voxel whose mean is exactly that.  With f = 128: u = 128 * 0.25 / 4 + cx = 8 + cx, v = cy, dv16 = 128 B / 4 * 16 = 512 B,
    h = 128 * 0.25 / 4 * 0.5 = 4."""
    W, H = R.W, R.H
    P = _one(0.25, 0.0, 4.0)
    cam = lambda f=128.0, cx=72.0, cy=40.0, b=0.5: (f, cx, cy, b)
    full = 81  # a whole footprint of r = 4
    out = {
        # dv16 + 0.5 on an integer: 256.5 rounds up; the double below it does not
        "dv16_half": (P, cam(b=0.5 + 1.0 / 1024), _unit(), 1, 8, (1, 1, full, full), [(80, 40, 4, 257)]),
        "dv16_under_half": (P, cam(b=_below(0.5 + 1.0 / 1024)), _unit(), 1, 8, (1, 1, full, full), [(80, 40, 4, 256)]),
        # d16 = 1 is the smallest that is drawn, 32767 the largest
        "d16_1": (P, cam(b=1.0 / 1024), _unit(), 1, 8, (1, 1, full, full), [(80, 40, 4, 1)]),
        # dv16 = 0.5 - 2^-54: the f64 sum dv16 + 0.5 rounds to 1.0, so the rule as stated still draws it; 0.5 - 2^-53 it does not
        "d16_1_by_the_sum": (P, cam(b=_below(1.0 / 1024)), _unit(), 1, 8, (1, 1, full, full), [(80, 40, 4, 1)]),
        "d16_0": (P, cam(b=_below(_below(1.0 / 1024))), _unit(), 1, 8, (1, 0, 0, 0), []),
        "d16_32767": (P, cam(b=_below(32767.5 / 512)), _unit(), 1, 8, (1, 1, full, full), [(80, 40, 4, 32767)]),
        "d16_32768": (P, cam(b=32767.5 / 512), _unit(), 1, 8, (1, 0, 0, 0), []),
        # h + 0.5 on an integer: f = 144 gives h = 4.5, r = 5 (u = 9 + cx); the double below gives 4
        "h_half": (P, cam(f=144.0), _unit(), 1, 8, (1, 1, 121, 121), [(81, 40, 5, 288)]),
        "h_under_half": (P, cam(f=_below(144.0)), _unit(), 1, 8, (1, 1, full, full), [(81, 40, 4, 288)]),
        "r_cut_by_max_radius": (P, cam(), _unit(), 1, 2, (1, 1, 25, 25), [(80, 40, 2, 256)]),
        "r_zero": (P, cam(), _unit(), 1, 0, (1, 1, 1, 1), [(80, 40, 0, 256)]),
        "r_sixteen": (P, cam(f=512.0, cx=48.0), _unit(), 1, 16, (1, 1, 33 * 33, 33 * 33), [(80, 40, 16, 1024)]),
        # the footprint against the image's edges: the last column or row, then nothing
        "px_minus_r": (P, cam(cx=-12.0), _unit(), 1, 8, (1, 1, 9, 9), [(-4, 40, 4, 256)]),
        "px_minus_r_minus_1": (P, cam(cx=-13.0), _unit(), 1, 8, (1, 0, 0, 0), []),
        "px_width_minus_1_plus_r": (P, cam(cx=W - 1 + 4 - 8.0), _unit(), 1, 8, (1, 1, 9, 9), [(W + 3, 40, 4, 256)]),
        "px_width_plus_r": (P, cam(cx=W + 4 - 8.0), _unit(), 1, 8, (1, 0, 0, 0), []),
        "py_minus_r": (P, cam(cy=-4.0), _unit(), 1, 8, (1, 1, 9, 9), [(80, -4, 4, 256)]),
        "py_minus_r_minus_1": (P, cam(cy=-5.0), _unit(), 1, 8, (1, 0, 0, 0), []),
        "py_height_minus_1_plus_r": (P, cam(cy=H + 3.0), _unit(), 1, 8, (1, 1, 9, 9), [(80, H + 3, 4, 256)]),
        "py_height_plus_r": (P, cam(cy=H + 4.0), _unit(), 1, 8, (1, 0, 0, 0), []),
        "corner": (P, cam(cx=-12.0, cy=-4.0), _unit(), 1, 8, (1, 1, 1, 1), [(-4, -4, 4, 256)]),
        # u = -4.5 exactly rounds up to -4; the double below it rounds to -5, outside
        "u_half": (P, cam(cx=-12.5), _unit(), 1, 8, (1, 1, 9, 9), [(-4, 40, 4, 256)]),
        "u_under_half": (P, cam(cx=float(np.nextafter(-12.5, -13.0))), _unit(), 1, 8, (1, 0, 0, 0), []),
        "c2_zero": (P, cam(), _unit(tz=-4.0), 1, 8, (1, 0, 0, 0), []),
        "c2_negative": (P, cam(), _unit(tz=-5.0), 1, 8, (1, 0, 0, 0), []),
        # c_2 = 4e-310: dv16 overflows for both voxels, u for the first as well
        "c2_tiny": (np.concatenate([P, _one(0.0, 0.0, 4.0)]), cam(), _unit(z_scale=1e-310), 1, 8, (2, 0, 0, 0), []),
        # two voxels on one pixel, in either order of the table: the nearer one stays
        "nearer_over_farther": (np.concatenate([_one(0.0, 0.0, 8.0, 0xF0), _one(0.0, 0.0, 4.0, 0x10)]), cam(), _unit(), 1, 0, (2, 2, 2, 1),
                                [(72, 40, 0, 256), (72, 40, 0, 128)]),
        "nearer_over_farther_2": (np.concatenate([_one(0.0, 0.0, 2.0, 0x10), _one(0.0, 0.0, 4.0, 0xF0)]), cam(), _unit(), 1, 0, (2, 2, 2, 1),
                                  [(72, 40, 0, 512), (72, 40, 0, 256)]),
        # the same with their footprints: r = 2 at 8 m inside r = 4 at 4 m, and r = 8 (cut from 8) at 2 m over r = 4
        "radii_2_in_4": (np.concatenate([_one(0.0, 0.0, 8.0, 0xF0), _one(0.0, 0.0, 4.0, 0x10)]), cam(), _unit(), 1, 8, (2, 2, 81 + 25, 81),
                         [(72, 40, 4, 256), (72, 40, 2, 128)]),
        "radii_8_over_4": (np.concatenate([_one(0.0, 0.0, 2.0, 0x10), _one(0.0, 0.0, 4.0, 0xF0)]), cam(), _unit(), 1, 8, (2, 2, 289 + 81, 289),
                           [(72, 40, 8, 512), (72, 40, 4, 256)]),
        # neighbours at one depth share the column between them: the larger mean intensity stays, whichever comes first
        "equal_d16": (np.concatenate([_one(0.0, 0.0, 4.0, 0x90), _one(0.25, 0.0, 4.0, 0x20)]), cam(), _unit(), 1, 8, (2, 2, 162, 153),
                      [(72, 40, 4, 256), (80, 40, 4, 256)]),
        "equal_d16_2": (np.concatenate([_one(0.0, 0.0, 4.0, 0x20), _one(0.25, 0.0, 4.0, 0x90)]), cam(), _unit(), 1, 8, (2, 2, 162, 153),
                        [(72, 40, 4, 256), (80, 40, 4, 256)]),
        "count_is_min_count": (_one(0.25, 0.0, 4.0, n=3), cam(), _unit(), 3, 8, (1, 1, full, full), [(80, 40, 4, 256)]),
        "count_below_min_count": (_one(0.25, 0.0, 4.0, n=2), cam(), _unit(), 3, 8, (0, 0, 0, 0), []),
        "mean_intensity_is_floored": (np.concatenate([_one(0.25, 0.0, 4.0, 0x11), _one(0.25, 0.0, 4.0, 0x12)]), cam(), _unit(), 1, 0,
                                      (1, 1, 1, 1), [(80, 40, 0, 256)]),
    }
    return out


def _single_want(name):
    p, cam, m, min_count, max_radius, counts, drawn = singles()[name]
    t = V.insert_np(p, IDENT, 0.25)
    return t, RR.render_np(t, R.W, R.H, cam, m, 0.25, min_count, max_radius)


# ===================================================================================================== CPU
def test_the_two_routes_of_the_restatement_agree_on_every_scene():
    for vs, _ in SIZES:
        t = table_a(vs)
        for view, (m, _) in VIEWS.items():
            for max_radius in RADII:
                for min_count in MIN_COUNTS:
                    a = want(vs, view, max_radius, min_count)
                    assert _same(a, RR.render_py(t, R.W, R.H, R.CAM, m, vs, min_count, max_radius)), (vs, view, max_radius, min_count)
                    assert a[2][0] == int(((t.ci >> np.uint64(40)) >= np.uint64(min_count)).sum()) and a[2][3] == int((a[0] > 0).sum())
                    assert ((a[0] == RR.FILTERED) == (a[0] <= 0)).all() and not a[1][a[0] <= 0].any()
    for shape in SHAPES:
        a = want(0.1, "B", 8, 1, shape)
        assert _same(a, RR.render_py(table_a(0.1), shape[0], shape[1], _scaled_cam(*shape), W2B, 0.1)), shape
        assert a[0].shape == shape[::-1] and a[2][3] >= 1
    for name, (p, cam, m, min_count, max_radius, counts, drawn) in singles().items():
        t, a = _single_want(name)
        assert _same(a, RR.render_py(t, R.W, R.H, cam, m, 0.25, min_count, max_radius)), name
        # and both give what the scene was built to give
        assert a[2] == counts and [d[:4] for d in RR.render_py.last] == drawn, (name, a[2], RR.render_py.last)


def test_the_main_scene_is_what_the_comparisons_need():
    da = scene()[1]
    table = {}
    for vs, _ in SIZES:
        a, b = want(vs, "A"), want(vs, "B")
        table[vs] = (a[2][1], a[2][0], int((a[0] == RR.FILTERED).sum()), b[2][1])
        # one pixel per voxel: what is drawn is the measured map, up to the scene's noise of 0..2 sixteenths
        z = want(vs, "A", 0)
        hit = z[0] > 0
        assert hit.sum() >= 1000 and np.abs(z[0].astype(np.int64) - da.astype(np.int64))[hit].max() <= 2, vs
        assert z[2][2] == z[2][1]  # one max operation per drawn voxel
        # a map never carves itself through its own render: d16 = floor(dv16 + 0.5) > dv16 - 1, and the pixel holds a maximum
        for view, (m, _) in VIEWS.items():
            r = want(vs, view)
            assert R.carve_np(table_a(vs), r[0], R.CAM, m, vs, 0, 1, 0)[1][2] == 0, (vs, view)
            assert R.carve_np(table_a(vs), r[0], R.CAM, m, vs, 0, 0, 0)[1][2] >= 300, (vs, view)
    assert table == {0.05: (10903, 10903, 0, 10186), 0.1: (5239, 5239, 4, 5011), 0.25: (1376, 1376, 0, 1322)}, table
    assert [R.carve_np(table_a(vs), want(vs, "A")[0], R.CAM, W2A, vs, 0, 0, 0)[1][2] for vs, _ in SIZES] == [8165, 2134, 359]
    RR.render_py(table_a(0.25), R.W, R.H, R.CAM, W2A, 0.25)
    assert {d[2] for d in RR.render_py.last} == {2, 3, 5}
    for vs, _ in SIZES:  # min_count 3 takes voxels away, and view B loses what A never saw
        assert 0 < want(vs, "A", 8, 3)[2][0] < want(vs, "A")[2][0] and (want(vs, "B")[0] == RR.FILTERED).sum() >= 500


def test_every_misreading_of_the_contract_changes_a_render():
    got = {}
    for variant, (vs, view, min_count, _) in MISREADINGS.items():
        right = want(vs, view, 8, min_count)
        wrong = RR.render_np(table_a(vs), R.W, R.H, R.CAM, VIEWS[view][0], vs, min_count, 8, variant=variant)
        got[variant] = int(((right[0] != wrong[0]) | (right[1] != wrong[1])).sum())
        assert got[variant] > 0, variant
    assert set(got) == set(RR.VARIANTS)
    assert got == {k: v[3] for k, v in MISREADINGS.items()}, got


def test_pure_entries_and_refusals_without_a_context():
    from stereo_vo_amd import api
    L = api.lib()
    d = api.voxel_render_default_params()
    assert (d.min_count, d.max_radius) == (1, 8)
    assert L.svo_voxel_render_default_params(None) == -1
    assert api.voxel_render_workspace_bytes(1241, 376) == 4 * 1241 * 376 and api.voxel_render_workspace_bytes(1, 1) == 4
    assert api.voxel_render_workspace_bytes(0, 5) == 0 and api.voxel_render_workspace_bytes(5, -1) == 0
    assert api.voxel_render_workspace_bytes(40000, 40000) == 4 * 40000 * 40000  # past 2^32
    buf = (C.c_double * 12)()
    cam = _cam()
    # a null map is refused by every entry
    assert L.svo_voxel_map_render_dev(None, 16, 16, C.byref(cam), buf, C.byref(d), buf, buf, buf, None) == -1
    assert L.svo_voxel_map_render_pose7_dev(None, 16, 16, C.byref(cam), buf, C.byref(d), buf, buf, buf, None) == -1
    assert L.svo_voxel_map_render(None, 16, 16, C.byref(cam), buf, C.byref(d), buf, buf, None) == -1
    assert L.svo_voxel_render_set_mode(None, 1, 1) == -1


# ===================================================================================================== GPU
def _render(vm, w, h, cam4, m12, max_radius, min_count, how, intensity=True, counts=True, offset=0):
    """One render by the named entry: (disp16, intensity or None, counts or None).  offset: bytes by which the device outputs are
    moved off their natural alignment."""
    import torch
    from stereo_vo_amd import api
    cam = api.CameraInfo(cam4[0], cam4[1], cam4[2], 0, 0, 0, 0, cam4[3])
    if how == "host":
        d, g, c = vm.render_host(w, h, cam, w2c12=m12, max_radius=max_radius, min_count=min_count)
        return d, g, (c["n_qualifying"], c["n_drawn"], c["n_splat"], c["n_pixels"])
    n = w * h
    ws = torch.full((n + 4,), 0x7F7F7F7F, dtype=torch.int32, device="cuda")  # a dirty workspace: the call clears it
    dd = torch.full((n + 8,), 0x5555, dtype=torch.int16, device="cuda")
    gg = torch.full((n + 16,), 0xAA, dtype=torch.uint8, device="cuda")
    cnt = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    wp, dp, gp = ws.data_ptr() + (4 if offset else 0), dd.data_ptr() + (2 if offset else 0), gg.data_ptr() + (1 if offset else 0)
    kw = dict(max_radius=max_radius, min_count=min_count, workspace_ptr=wp, disp_ptr=dp, intensity_ptr=gp if intensity else None,
              counts_ptr=cnt.data_ptr() if counts else None)
    if how == "pose7":
        assert np.array_equal(np.asarray(m12).reshape(3, 4)[:, :3], np.eye(3))
        out = vm.render(w, h, cam, pose7=np.concatenate([[1.0, 0, 0, 0], np.asarray(m12).reshape(3, 4)[:, 3]]), **kw)
    else:
        out = vm.render(w, h, cam, w2c12=m12, **kw)
    assert out["disp16"] == dp and out["width"] == w and out["height"] == h
    vm.ctx.sync()  # the tensors go out of scope behind the return
    o = 1 if offset else 0
    d_all, g_all = dd.cpu().numpy(), gg.cpu().numpy()
    assert (d_all[:o] == 0x5555).all() and (d_all[o + n:] == 0x5555).all()  # nothing beside the outputs is written
    assert (g_all[:o] == 0xAA).all() and (g_all[o + n:] == 0xAA).all()
    g = g_all[o:o + n].reshape(h, w)
    if not intensity:
        assert (g == 0xAA).all()
    c = tuple(cnt.cpu().tolist())
    if not counts:
        assert c == (-1, -1, -1, -1)
    return d_all[o:o + n].reshape(h, w), g if intensity else None, c if counts else None


def _filled(ctx, vs, lg, pts=None):
    t = table_a(vs)
    _fits(t.keys, lg)
    vm = _map(ctx, vs, lg)
    _insert(vm, scene()[0] if pts is None else pts, A2W)
    return vm


@pytest.mark.gpu
@pytest.mark.parametrize("view", ("A", "B"))
@pytest.mark.parametrize("vs,lg", SIZES)
def test_main_scene(ctx, vs, lg, view):
    vm = _filled(ctx, vs, lg)
    before = vm.download()
    for max_radius in RADII:
        for min_count in MIN_COUNTS:
            for how in ("dev", "pose7", "host"):
                got = _render(vm, R.W, R.H, R.CAM, VIEWS[view][0], max_radius, min_count, how)
                assert _same(got, want(vs, view, max_radius, min_count)), (max_radius, min_count, how)
    after = vm.download()
    assert all(np.array_equal(before[k], after[k]) for k in before)  # the map is only read
    vm.close()


@pytest.mark.gpu
def test_null_intensity_and_null_counts(ctx):
    vs, lg = 0.1, 14
    vm = _filled(ctx, vs, lg)
    w = want(vs, "B")
    d, g, c = _render(vm, R.W, R.H, R.CAM, W2B, 8, 1, "dev", intensity=False)
    assert g is None and np.array_equal(d, w[0]) and c == w[2]
    d, g, c = _render(vm, R.W, R.H, R.CAM, W2B, 8, 1, "pose7", counts=False)
    assert c is None and np.array_equal(d, w[0]) and np.array_equal(g, w[1])
    d, g, c = _render(vm, R.W, R.H, R.CAM, W2B, 8, 1, "dev", intensity=False, counts=False)
    assert g is None and c is None and np.array_equal(d, w[0])
    from stereo_vo_amd import api
    L, cam, prm, m = ctx.L, _cam(), api.voxel_render_default_params(), np.ascontiguousarray(W2B)
    d = np.empty((R.H, R.W), np.int16)
    assert L.svo_voxel_map_render(vm.h, R.W, R.H, C.byref(cam), m.ctypes.data_as(C.c_void_p), C.byref(prm), d.ctypes.data_as(C.c_void_p), None, None) == 0
    assert np.array_equal(d, w[0])
    vm.close()


@pytest.mark.gpu
def test_record_order_and_drawing_mode_change_no_bit(ctx):
    for vs, lg in ((0.05, 15), (0.25, 14)):
        vm = _filled(ctx, vs, lg, scene()[0][::-1].copy())
        for view in VIEWS:
            assert _same(_render(vm, R.W, R.H, R.CAM, VIEWS[view][0], 8, 1, "dev"), want(vs, view)), (vs, view)
        for coop, pre in ((False, False), (False, True), (True, False), (True, True)):
            vm.render_set_mode(coop, pre)
            assert _same(_render(vm, R.W, R.H, R.CAM, W2A, 8, 1, "dev"), want(vs, "A")), (vs, coop, pre)
        vm.close()


@pytest.mark.gpu
def test_render_after_a_carve_draws_no_carved_voxel(ctx):
    _, _, _, db = scene()
    vs, lg = 0.05, 15
    vm = _filled(ctx, vs, lg)
    carved, counts = R.carve_np(table_a(vs), db, R.CAM, W2B, vs)
    assert counts[2] >= 300
    c = vm.carve_host(db, _cam(), w2c12=W2B)
    assert c["n_carved"] == counts[2]
    for view, (m, _) in VIEWS.items():
        w = RR.render_np(carved, R.W, R.H, R.CAM, m, vs)
        assert w[2][0] == len(table_a(vs).keys) - counts[2] and not _same(w, want(vs, view))
        assert _same(_render(vm, R.W, R.H, R.CAM, m, 8, 1, "dev"), w), view
    vm.close()


@pytest.mark.gpu
@pytest.mark.parametrize("vs,lg", SIZES)
def test_a_map_never_carves_itself_through_its_own_render(ctx, vs, lg):
    import torch
    vm = _filled(ctx, vs, lg)
    cam = _cam()
    n = R.W * R.H
    ws, dd = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int16, device="cuda")
    cnt = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for view, (m, _) in VIEWS.items():
        for margin, none in ((1, True), (0, False)):  # margin16 0 last: it does carve
            out = vm.render(R.W, R.H, cam, w2c12=m, workspace_ptr=ws.data_ptr(), disp_ptr=dd.data_ptr())
            vm.carve(out["disp16"], R.W, R.H, cam, w2c12=m, radius=0, margin16=margin, counts_ptr=cnt.data_ptr())
            vm.ctx.sync()
            got = tuple(cnt.cpu().tolist())
            if none:
                assert got[2] == 0 and got[1] >= 1000, (view, got)
            else:
                assert got == R.carve_np(table_a(vs), want(vs, view)[0], R.CAM, m, vs, 0, 0, 0)[1] and got[2] >= 300, (view, got)
                vm.clear()
                _insert(vm, scene()[0], A2W)
    vm.close()


@pytest.mark.gpu
def test_the_render_is_an_input_of_the_cloud_launch(ctx):
    import torch
    from stereo_vo_amd import api
    from test_dense_cloud import _expected_cloud, _same as same_records
    vs, lg, step = 0.1, 14, 2
    vm = _filled(ctx, vs, lg)
    cam = _cam()
    n, mp = R.W * R.H, (R.W // step) * (R.H // step)
    ws, dd = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int16, device="cuda")
    gg = torch.zeros(n, dtype=torch.uint8, device="cuda")
    pts = torch.zeros(mp * 4, dtype=torch.int32, device="cuda")
    cnt = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    out = vm.render(R.W, R.H, cam, pose7=POSE_B, workspace_ptr=ws.data_ptr(), disp_ptr=dd.data_ptr(), intensity_ptr=gg.data_ptr())
    ctx.disparity_cloud(out["disp16"], out["intensity"], 1, R.W, R.H, R.W, n, cam, None, api.CloudParams(step, 0.0, mp), pts.data_ptr(),
                        cnt.data_ptr())
    ctx.sync()
    disp, inten = dd.cpu().numpy().reshape(R.H, R.W), gg.cpu().numpy().reshape(R.H, R.W)
    assert np.array_equal(disp, want(vs, "B")[0]) and np.array_equal(inten, want(vs, "B")[1])
    ref = _expected_cloud(inten, disp, cam, step, 0.0, None)
    n_total, n_stored = cnt.cpu().tolist()
    assert n_total == n_stored == len(ref) == int((disp[::step, ::step] > 0).sum()) >= 1000
    assert n_total < mp  # the FILTERED pixels of view B give no point
    assert same_records(ref, pts.cpu().numpy().view(api.CLOUD_POINT_DTYPE)[:n_stored])
    vm.close()


@pytest.mark.gpu
def test_image_sizes_that_reach_the_tail_of_the_resolve(ctx):
    vs, lg = 0.1, 14
    vm = _filled(ctx, vs, lg)
    for shape in SHAPES:
        for offset in (0, 1):  # 1: pointers the vector accesses cannot take
            got = _render(vm, shape[0], shape[1], _scaled_cam(*shape), W2B, 8, 1, "dev", offset=offset)
            assert _same(got, want(vs, "B", 8, 1, shape)), (shape, offset)
        assert _same(_render(vm, shape[0], shape[1], _scaled_cam(*shape), W2B, 8, 1, "host"), want(vs, "B", 8, 1, shape)), shape
    vm.close()


@pytest.mark.gpu
def test_constructed_single_voxels_in_a_table_smaller_than_one_tile(ctx):
    vm = _map(ctx, 0.25, 8)  # 256 slots: one workgroup walks 2,048
    for i, (name, (p, cam, m, min_count, max_radius, counts, drawn)) in enumerate(sorted(singles().items())):
        t, w = _single_want(name)
        assert w[2] == counts, name
        vm.clear()
        _insert(vm, p, IDENT)
        vm.render_set_mode(i % 4 < 2, i % 2 == 0)
        assert _same(_render(vm, R.W, R.H, cam, m, max_radius, min_count, ("dev", "host")[i % 2]), w), name
    vm.close()


@pytest.mark.gpu
def test_bad_arguments_launch_nothing_and_leave_the_map_usable(ctx):
    import torch
    from stereo_vo_amd import api
    L = ctx.L
    vs, lg = 0.25, 11
    vm = _filled(ctx, vs, lg)
    n = R.W * R.H
    ws, dd = torch.zeros(n + 1, dtype=torch.int32, device="cuda"), torch.full((n,), 0x5555, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    cam, m, q = _cam(), np.ascontiguousarray(W2B), np.ascontiguousarray(POSE_B)
    mp, qp = m.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p)
    P = api.VoxelRenderParams
    host = np.full((R.H, R.W), 0x5555, np.int16)
    dev = lambda **k: L.svo_voxel_map_render_dev(vm.h, k.get("w", R.W), k.get("h", R.H), k.get("cam", C.byref(cam)), k.get("m", mp),
                                                 k.get("prm", C.byref(k.get("P", P(1, 8)))), k.get("ws", ws.data_ptr()),
                                                 k.get("disp", dd.data_ptr()), None, None)
    bad_cam = lambda f, b: C.byref(api.CameraInfo(f, 80, 40, 0, 0, 0, 0, b))
    inf, nan = float("inf"), float("nan")
    ctx.profile_select("voxel_render")
    calls = [(lambda: dev(cam=None), "cam"), (lambda: dev(m=None), "w2c12"), (lambda: dev(prm=None), "params"), (lambda: dev(ws=None), "workspace"),
             (lambda: dev(ws=ws.data_ptr() + 2), "workspace"), (lambda: dev(disp=None), "disp16"),
             (lambda: dev(P=P(0, 8)), "min_count"), (lambda: dev(P=P(-3, 8)), "min_count"),
             (lambda: dev(P=P(1, -1)), "max_radius"), (lambda: dev(P=P(1, 17)), "max_radius"),
             (lambda: dev(w=0), "width"), (lambda: dev(h=0), "height"), (lambda: dev(w=1281), "width"), (lambda: dev(h=721), "height"),
             (lambda: dev(cam=bad_cam(0.0, 0.5)), "focal"), (lambda: dev(cam=bad_cam(-120.0, 0.5)), "focal"), (lambda: dev(cam=bad_cam(inf, 0.5)), "focal"),
             (lambda: dev(cam=bad_cam(nan, 0.5)), "focal"), (lambda: dev(cam=bad_cam(120.0, 0.0)), "baseline"),
             (lambda: dev(cam=bad_cam(120.0, -0.5)), "baseline"), (lambda: dev(cam=bad_cam(120.0, inf)), "baseline"),
             (lambda: dev(cam=bad_cam(120.0, nan)), "baseline"),
             (lambda: L.svo_voxel_map_render_pose7_dev(vm.h, R.W, R.H, C.byref(cam), None, C.byref(P(1, 8)), ws.data_ptr(), dd.data_ptr(), None, None), "pose7"),
             (lambda: L.svo_voxel_map_render(vm.h, R.W, R.H, C.byref(cam), mp, C.byref(P(1, 8)), None, None, None), "disp16"),
             (lambda: L.svo_voxel_map_render(vm.h, R.W, R.H, C.byref(cam), mp, C.byref(P(1, 99)), host.ctypes.data_as(C.c_void_p), None, None), "max_radius")]
    for call, word in calls:
        assert call() == -1 and word in L.svo_last_error(ctx.h).decode(), word
    assert ctx.profile_read()[1] == 0
    assert (dd.cpu().numpy() == 0x5555).all() and (host == 0x5555).all()
    assert dev(w=1, h=1) == 0  # the smallest image is taken
    assert ctx.profile_read()[1] == 1
    ctx.profile_select(None)
    with pytest.raises(ValueError):
        vm.render(R.W, R.H, cam, workspace_ptr=ws.data_ptr(), disp_ptr=dd.data_ptr())
    with pytest.raises(ValueError):
        vm.render_host(R.W, R.H, cam, w2c12=m, pose7=q)
    # the map is what it was, and renders
    t = table_a(vs)
    d = vm.download()
    occ = d["keys"] != np.uint64(V.EMPTY)
    o = np.argsort(d["keys"][occ])
    assert all(np.array_equal(d[k][occ][o], getattr(t, k)) for k in ("keys", "ci", "sx", "sy", "sz"))
    assert _same(_render(vm, R.W, R.H, R.CAM, W2B, 8, 1, "pose7"), want(vs, "B"))
    vm.close()
