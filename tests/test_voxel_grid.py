"""The voxel map's grid (include/svo.h, "Voxel map grid") against its restatement tests/voxel_grid_ref.py, with == on the class,
the intensity, the two tallies and the five counts, and on top and bottom as bit patterns.

CPU: the restatement's two routes agree on every scene and parameter set used below; the street scene's figures and the facts the
comparisons stand on are asserted on the restatement; each deliberate misreading of the contract changes a grid; the pure entries,
svo_voxel_grid_cell_of at every boundary and the refusals that need no context; stereo_vo_amd/host/voxel_args.h's grid part walked by
tests/sanitize/voxel_grid_args_test.cpp under ASan + UBSan.
GPU: the street scene through the _dev and the host entry; every optional output left out; record order; other orientations; grid
shapes that reach the resolve's tail; both modes of the walk (svo_voxel_grid_set_mode); a table shorter than one workgroup's tile; the grid after a carve and after a removal;
constructed voxels; bad calls.  Every device call runs into a dirty workspace and sentinel-filled outputs whose guard elements stay.

The scene "street" (34,524 records 0.06 m apart, identity transform, y down): a road with a kerb, a box, a wall, an overhang above the
band and a thin post; 32 x 13 cells of 0.5 m from z = 0, x = -3.2, the band -2.5 .. 2.0, step 0.3.  On the restatement:

  voxel size  voxels  capacity_log2  longest_run  counts at min_count 1            at min_count 2                   UNKNOWN/LEVEL/OBSTACLE
  0.05        34,491  16             49           (34491, 33913, 27414, 312, 19)   (33, 33, 32, 4, 2)               104 / 293 / 19
  0.1         13,040  15             24           (13040, 12840, 10406, 312, 19)   (10919, 10737, 8685, 312, 19)    104 / 293 / 19
  0.25         2,074  13             16           (2074, 2042, 1665, 312, 21)      (2057, 2025, 1649, 312, 21)      104 / 291 / 21

Misreadings at 0.1 m, cells of 416 that change: band ignored 10 classes; hgt = g without the sign 312 tops; truncating cell division
24 n_voxels; height from the key alone 312 tops (0 classes); count > min_count 312 n_voxels; a and b swapped 312 classes; mean of all
intensities 308 intensities; span >= step changes nothing in the street and 1 class of the constructed pair "span_step".
"""
import ctypes as C
import functools

import numpy as np
import pytest

import voxel_carve_ref as R
import voxel_grid_ref as G
import voxel_ref as V
from test_host_sanitizers import _run_sanitized
from test_voxel_map import IDENT, _dev, _fits, _insert, _map, _stored

FIGURES = {  # voxel size -> (voxels, longest_run, counts at min_count 1, at min_count 2, (UNKNOWN, LEVEL, OBSTACLE) at min_count 1)
    0.05: (34491, 49, (34491, 33913, 27414, 312, 19), (33, 33, 32, 4, 2), (104, 293, 19)),
    0.1: (13040, 24, (13040, 12840, 10406, 312, 19), (10919, 10737, 8685, 312, 19), (104, 293, 19)),
    0.25: (2074, 16, (2074, 2042, 1665, 312, 21), (2057, 2025, 1649, 312, 21), (104, 291, 21))}
MISREADINGS = {"no_band": ("cls", 10), "no_sign": ("top", 312), "trunc_cell": ("n_voxels", 24), "key_height": ("top", 312),
               "count_gt": ("n_voxels", 312), "swap_ab": ("cls", 312), "mean_intensity": ("intensity", 308)}  # at 0.1 m; span_ge: see the test
MID = (0.1, 15, 5)
# the same table seen with x up and with z up; na != nb makes a swap of the axes visible
ORIENTATIONS = {"x_up": G.Params(0, 1, -3.0, 1.0, 5, 11, 27, -2.0, 3.0, 0.3, 1), "z_up": G.Params(2, 1, -4.2, -3.0, 5, 17, 10, 0.0, 13.0, 1.0, 1)}
# one cell over everything; a tail behind the resolve's wavefronts and an odd cell size; a multiple of the wavefront and of the workgroup
SHAPES = {"1x1": G.street_params(1024)._replace(origin_a=-50.0, origin_b=-50.0, na=1, nb=1),
          "7x5": G.street_params(23)._replace(origin_a=1.0, origin_b=-4.5, na=7, nb=5),
          "64x64": G.street_params(2)._replace(origin_a=2.0, origin_b=-6.4, na=64, nb=64)}
CARVE_VS, CARVE_LG = 0.1, 14
CARVE_PARAMS = G.Params(1, -1, 2.0, -4.0, 5, 14, 16, -3.0, 3.0, 0.3, 1)  # over tests/voxel_carve_ref.py's scene
OUTPUTS = ("top", "bottom", "intensity", "n_voxels", "n_points")


@functools.lru_cache(maxsize=None)
def street():
    p = G.street()
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def table(vs):
    return V.insert_np(street(), IDENT, vs)


@functools.lru_cache(maxsize=None)
def want(vs, prm):
    g = G.grid_np(table(vs), prm, vs)
    for a in g[:6]:
        a.setflags(write=False)
    return g


def _box_region(p):
    """The records of the box and of the road under and around it."""
    return (p["x"] >= -1.2) & (p["x"] < 0.0) & (p["z"] >= 4.9) & (p["z"] < 6.1)


def _carve_scene():
    from test_voxel_carve import A2W, W2B, scene, table_a
    return scene(), table_a(CARVE_VS), A2W, W2B


def _classes(g):
    return tuple(int((g.cls == k).sum()) for k in (G.UNKNOWN, G.LEVEL, G.OBSTACLE))


# ===================================================================================================== CPU
def test_the_two_routes_of_the_restatement_agree_on_every_scene_and_parameter_set():
    for vs, lg, cv in G.STREET_SIZES:
        for min_count in (1, 2):
            prm = G.street_params(cv, min_count)
            assert G.same(want(vs, prm), G.grid_py(table(vs), prm, vs)), (vs, min_count)
    vs = MID[0]
    for name, prm in {**ORIENTATIONS, **SHAPES}.items():
        a = want(vs, prm)
        assert G.same(a, G.grid_py(table(vs), prm, vs)), name
        assert a.cls.shape == (prm.na, prm.nb) and a.counts[2] >= 100 and a.counts[3] >= 1, (name, a.counts)
    assert all(_classes(want(vs, p))[1] and _classes(want(vs, p))[2] for p in ORIENTATIONS.values())  # level and obstacle cells either way
    assert want(vs, SHAPES["1x1"]).counts[2] == want(vs, SHAPES["1x1"]).counts[1] == int(want(vs, SHAPES["1x1"]).n_voxels[0, 0])
    # infinite bounds take every height; a grid far away takes nothing
    wide = G.street_params(5)._replace(up_lo=-np.inf, up_hi=np.inf)
    assert G.same(want(vs, wide), G.grid_py(table(vs), wide, vs)) and want(vs, wide).counts[1] == want(vs, wide).counts[0]
    far = G.street_params(5)._replace(origin_a=1e300, origin_b=-1e300)
    assert G.same(want(vs, far), G.grid_py(table(vs), far, vs)) and want(vs, far).counts[2:] == (0, 0, 0)
    # the table after a carve, with its zero-count keys
    (_, _, _, db), t, _, W2B = _carve_scene()
    carved, counts = R.carve_np(t, db, R.CAM, W2B, CARVE_VS)
    assert counts[2] >= 50
    for tab in (t, carved):
        a = G.grid_np(tab, CARVE_PARAMS, CARVE_VS)
        assert G.same(a, G.grid_py(tab, CARVE_PARAMS, CARVE_VS)) and a.counts[0] == int(((tab.ci >> np.uint64(40)) >= 1).sum())
        assert a.counts[3] >= 20 and _classes(a)[2] >= 1
    assert not G.same(G.grid_np(t, CARVE_PARAMS, CARVE_VS), G.grid_np(carved, CARVE_PARAMS, CARVE_VS))
    for name, (p, prm, facts) in G.constructed().items():
        t = V.insert_np(p, IDENT, G.CONSTRUCTED_VS)
        a = G.grid_np(t, prm, G.CONSTRUCTED_VS)
        assert G.same(a, G.grid_py(t, prm, G.CONSTRUCTED_VS)), name
        # and both give what the case was built to give
        cells = {k: v for k, v in facts.items() if k != "counts"}
        assert a.counts[:3] == facts["counts"] and a.counts[3] == len(cells), (name, a.counts)
        assert {divmod(c, prm.nb) for c in G.grid_py.last} == set(cells), name
        for at, (cls, htop, hbot, inten, nv, npt) in cells.items():
            got = (int(a.cls[at]), float(a.top[at]), float(a.bottom[at]), int(a.intensity[at]), int(a.n_voxels[at]), int(a.n_points[at]))
            assert got == (cls, htop / 65536.0 * 0.25, hbot / 65536.0 * 0.25, inten, nv, npt), (name, at, got)


def test_the_street_scene_is_what_the_comparisons_need():
    got = {}
    for vs, lg, cv in G.STREET_SIZES:
        t = table(vs)
        run = V.longest_run(V.occupied(t.keys, lg))
        assert run < V.MAX_PROBES, (vs, run)
        prm = G.street_params(cv)
        g = want(vs, prm)
        got[vs] = (len(t.keys), run, g.counts, want(vs, G.street_params(cv, 2)).counts, _classes(g))
        assert all(_classes(g))  # all three classes occur
        cells = G.street_cells(prm, vs)
        assert len(cells["kerb"]) >= 15 and len(cells["under_overhang"]) == 8 and len(cells["box"]) == 4 and len(cells["wall"]) == 13
        assert all(g.cls[c] == G.LEVEL for c in cells["kerb"] | cells["under_overhang"]), vs
        assert all(g.cls[c] == G.OBSTACLE for c in cells["box"] | cells["wall"] | cells["post"]), vs
        assert g.counts[1] < g.counts[0] and g.counts[2] < g.counts[1]  # the overhang is above the band, the road's edges are outside
        # the kerb is seen: its cells span more than the road's own slope and noise, and less than the step
        span = g.top - g.bottom
        assert all(0.08 < span[c] < 0.3 for c in cells["kerb"]) and span[4, 5] < 0.08
        assert t.n_rejected == 0 and t.n_inserted == len(street())
    assert got == FIGURES, got


def test_every_misreading_of_the_contract_changes_a_grid():
    vs, _, cv = MID
    prm = G.street_params(cv)
    right = want(vs, prm)
    got = {}
    for variant, (field, _) in MISREADINGS.items():
        wrong = G.grid_np(table(vs), prm, vs, variant=variant)
        got[variant] = (field, int((getattr(right, field) != getattr(wrong, field)).sum()))
        assert got[variant][1] > 0, variant
    assert got == MISREADINGS, got
    assert int((G.grid_np(table(vs), prm, vs, variant="key_height").cls != right.cls).sum()) == 0  # the fraction moves tops, not classes
    # span >= step changes nothing in the street; the constructed pair with a span of exactly step is its scene
    assert G.same(G.grid_np(table(vs), prm, vs, variant="span_ge"), right)
    p, cp, _ = G.constructed()["span_step"]
    t = V.insert_np(p, IDENT, G.CONSTRUCTED_VS)
    a, b = G.grid_np(t, cp, G.CONSTRUCTED_VS), G.grid_np(t, cp, G.CONSTRUCTED_VS, variant="span_ge")
    assert int((a.cls != b.cls).sum()) == 1 and a.cls[0, 0] == G.LEVEL and b.cls[0, 0] == G.OBSTACLE
    assert set(MISREADINGS) | {"span_ge"} == set(G.VARIANTS)


def _api_params(prm):
    from stereo_vo_amd import api
    return api.VoxelGridParams(*prm)


def test_pure_entries_cell_of_and_refusals_without_a_context():
    from stereo_vo_amd import api
    L = api.lib()
    d = api.voxel_grid_default_params(0.1)
    assert (d.up_axis, d.up_sign, d.cell_voxels, d.na, d.nb, d.min_count) == (1, -1, 5, 256, 256, 1)
    vs = float(np.float32(0.1))
    assert (d.origin_a, d.origin_b, d.up_lo, d.up_hi, d.obstacle_step) == (0.0, -128.0 * 5.0 * vs, -3.0, 2.5, 0.3)
    assert [api.voxel_grid_default_params(v).cell_voxels for v in (0.05, 0.25, 1.0, 3.0, 1e-4)] == [10, 2, 1, 1, 1024]
    assert L.svo_voxel_grid_default_params(C.c_float(0.1), None) == -1
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        assert L.svo_voxel_grid_default_params(C.c_float(bad), C.byref(api.VoxelGridParams())) == -1, bad
    assert api.voxel_grid_workspace_bytes(256, 256) == 32 * 256 * 256 and api.voxel_grid_workspace_bytes(1, 1) == 32
    assert api.voxel_grid_workspace_bytes(0, 5) == 0 and api.voxel_grid_workspace_bytes(5, -1) == 0
    assert api.voxel_grid_workspace_bytes(40000, 40000) == 32 * 40000 * 40000  # past 2^32
    # cell_of at every boundary: the restatement's rule, then the faces of the first and the last cell by hand
    for vs, _, cv in G.STREET_SIZES:
        prm = G.street_params(cv)
        p = _api_params(prm)
        for a in (-0.3, -1e-9, 0.0, 0.49, 0.5, 7.03, 15.99, 16.0, 16.2, 1e300, -1e300, float("inf")):
            for b in (-3.5, -3.26, -3.2, -3.1, 0.0, 1.03, 3.24, 3.26, 3.31, 99.0, float("-inf")):
                assert api.voxel_grid_cell_of(p, vs, a, b) == G.cell_of(prm, vs, a, b), (vs, a, b)
    p = _api_params(G.constructed_params())  # voxel 0.25, cells of 2 voxels from a = 0.25, b = -0.5, 3 x 2 of them
    below = lambda x: float(np.nextafter(x, -np.inf))
    assert api.voxel_grid_cell_of(p, 0.25, 0.25, -0.5) == (True, 0, 0) and api.voxel_grid_cell_of(p, 0.25, below(0.25), -0.5) == (False, -1, 0)
    assert api.voxel_grid_cell_of(p, 0.25, 0.25, below(-0.5)) == (False, 0, -1)
    assert api.voxel_grid_cell_of(p, 0.25, below(0.75), below(0.0)) == (True, 0, 0) and api.voxel_grid_cell_of(p, 0.25, 0.75, 0.0) == (True, 1, 1)
    assert api.voxel_grid_cell_of(p, 0.25, below(1.75), below(0.5)) == (True, 2, 1) and api.voxel_grid_cell_of(p, 0.25, 1.75, 0.0) == (False, 3, 1)
    assert api.voxel_grid_cell_of(p, 0.25, 1.0, 0.5) == (False, 1, 2)
    ia = C.c_int(77)
    assert L.svo_voxel_grid_cell_of(C.byref(p), C.c_float(0.25), C.c_double(1.0), C.c_double(0.0), None, C.byref(ia)) == 1 and ia.value == 1
    for call in (lambda: api.voxel_grid_cell_of(p, 0.25, float("nan"), 0.0), lambda: api.voxel_grid_cell_of(p, 0.25, 0.0, float("nan")),
                 lambda: api.voxel_grid_cell_of(p, 0.0, 0.0, 0.0), lambda: api.voxel_grid_cell_of(_api_params(G.constructed_params(na=0)), 0.25, 0.0, 0.0)):
        with pytest.raises(api.SvoError):
            call()
    assert L.svo_voxel_grid_cell_of(None, C.c_float(0.25), C.c_double(0.0), C.c_double(0.0), None, None) == -1
    # a null map is refused by both entries
    buf = (C.c_double * 12)()
    out = api.VoxelGridOut(C.addressof(buf))
    assert L.svo_voxel_map_grid_dev(None, C.byref(p), buf, C.byref(out), None) == -1
    assert L.svo_voxel_map_grid(None, C.byref(p), C.byref(out), None) == -1
    assert L.svo_voxel_grid_set_mode(None, 1) == -1


def test_voxel_grid_args_every_refusal_the_conversions_the_cell_rule_and_the_division(tmp_path):
    """host/voxel_args.h's grid part on the CPU under ASan + UBSan: every refusal at its boundary with code and exact message, the
    three conversions at +-clamp, with infinite bounds and negative origins, the floor division and cell_of at the grid's faces, the
    exact division against the 64-bit one (edges, the f32 round-up cases, a million seeded pairs), the defaults, the workspace size
    and the launch geometry without 32-bit wrap."""
    _run_sanitized(tmp_path, "voxel_grid_args_test", "voxel grid args ok")


# ===================================================================================================== GPU
_SENT = {"cls": (np.uint8, 0xAA), "top": (np.int32, 0x5555AAAA), "bottom": (np.int32, 0x3333CCCC), "intensity": (np.uint8, 0xBB),
         "n_voxels": (np.int32, 0x77777777), "n_points": (np.int64, 0x6666666666666666)}


def _grid(vm, prm, how="dev", skip=(), counts=True):
    """One grid by the named entry, as a G.Grid (None for an output in `skip`, and for counts when they are left out).  The device
    entry runs into a dirty workspace and sentinel-filled outputs, one guard element before and behind each."""
    import torch
    p = _api_params(prm)
    if how == "host":
        *arrays, c = vm.grid_host(p)
        return G.Grid(*arrays, tuple(c[k] for k in ("n_qualifying", "n_in_band", "n_binned", "n_cells", "n_obstacle")))
    n = prm.na * prm.nb
    ws = torch.full((4 * n + 2,), 0x7F7F7F7F7F7F7F7F, dtype=torch.int64, device="cuda")
    bufs = {k: torch.full((n + 2,), v, dtype=getattr(torch, np.dtype(t).name), device="cuda") for k, (t, v) in _SENT.items()}
    cnt = torch.full((7,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ptr = {k: None if k in skip else b.data_ptr() + b.element_size() for k, b in bufs.items()}
    out = vm.grid(p, workspace_ptr=ws.data_ptr() + 8, counts_ptr=cnt.data_ptr() + 8 if counts else None,
                  **{k + "_ptr": v for k, v in ptr.items()})
    assert out["cls"] == ptr["cls"] and (out["na"], out["nb"]) == (prm.na, prm.nb)
    vm.ctx.sync()  # the tensors go out of scope behind the return
    w = ws.cpu().numpy()
    assert w[0] == w[-1] == 0x7F7F7F7F7F7F7F7F
    got = {}
    for k, (t, v) in _SENT.items():
        a = bufs[k].cpu().numpy()
        assert a[0] == v and a[-1] == v, k  # nothing beside the outputs is written
        if k in skip:
            assert (a == v).all(), k
            got[k] = None
        else:
            got[k] = a[1:-1].reshape(prm.na, prm.nb)
    c = cnt.cpu().numpy()
    assert c[0] == c[-1] == -1 and (counts or (c == -1).all())
    # the workspace holds the four words of every cell
    cells = w[1:-1].view(np.uint64).reshape(n, 4)
    if got["n_voxels"] is not None:
        assert np.array_equal(cells[:, 2], got["n_voxels"].ravel().view(np.uint32))
    f32 = lambda a: None if a is None else a.view(np.float32)
    return G.Grid(got["cls"], f32(got["top"]), f32(got["bottom"]), got["intensity"], None if got["n_voxels"] is None else got["n_voxels"].view(np.uint32),
                  None if got["n_points"] is None else got["n_points"].view(np.uint64), tuple(int(v) for v in c[1:6]) if counts else None)


def _eq(got, w, what=""):
    for name in ("cls", "intensity", "n_voxels", "n_points"):
        if getattr(got, name) is not None:
            assert np.array_equal(getattr(got, name), getattr(w, name)), (what, name)
    for name in ("top", "bottom"):
        if getattr(got, name) is not None:
            assert np.array_equal(getattr(got, name).view(np.uint32), getattr(w, name).view(np.uint32)), (what, name)
    if got.counts is not None:
        assert tuple(got.counts) == tuple(w.counts), (what, got.counts, w.counts)


def _filled(ctx, vs, lg, pts=None):
    _fits(table(vs).keys, lg)
    vm = _map(ctx, vs, lg)
    _insert(vm, street() if pts is None else pts, IDENT)
    return vm


@pytest.mark.gpu
@pytest.mark.parametrize("vs,lg,cv", G.STREET_SIZES)
def test_street_scene(ctx, vs, lg, cv):
    vm = _filled(ctx, vs, lg)
    before = vm.download()
    for min_count in (1, 2):
        prm = G.street_params(cv, min_count)
        for how in ("dev", "host"):
            got = _grid(vm, prm, how)
            print(vs, min_count, how, "counts", got.counts, "classes", _classes(got))
            _eq(got, want(vs, prm), (min_count, how))
    after = vm.download()
    assert all(np.array_equal(before[k], after[k]) for k in before)  # the map is only read
    vm.close()


@pytest.mark.gpu
def test_every_optional_output_left_out(ctx):
    from stereo_vo_amd import api
    vs, lg, cv = MID
    vm = _filled(ctx, vs, lg)
    prm = G.street_params(cv)
    w = want(vs, prm)
    for skip in [(k,) for k in OUTPUTS] + [OUTPUTS]:
        got = _grid(vm, prm, skip=skip)
        assert all(getattr(got, k) is None for k in skip) and got.cls is not None
        _eq(got, w, skip)
    _eq(_grid(vm, prm, counts=False), w, "no counts")
    _eq(_grid(vm, prm, skip=OUTPUTS, counts=False), w, "cls alone")
    # the host entry with cls alone
    cls = np.full((prm.na, prm.nb), 0xAA, np.uint8)
    p = _api_params(prm)
    assert ctx.L.svo_voxel_map_grid(vm.h, C.byref(p), C.byref(api.VoxelGridOut(cls.ctypes.data)), None) == 0
    assert np.array_equal(cls, w.cls)
    vm.close()


@pytest.mark.gpu
def test_record_order_changes_no_bit(ctx):
    for vs, lg, cv in (G.STREET_SIZES[0], G.STREET_SIZES[2]):
        vm = _filled(ctx, vs, lg, street()[::-1].copy())
        for min_count in (1, 2):
            prm = G.street_params(cv, min_count)
            _eq(_grid(vm, prm), want(vs, prm), (vs, min_count))
        vm.close()


@pytest.mark.gpu
def test_both_modes_of_the_walk_give_the_same_bytes(ctx):
    import torch
    for vs, lg, cv in (G.STREET_SIZES[0], G.STREET_SIZES[2]):
        vm = _filled(ctx, vs, lg)
        prm = G.street_params(cv)
        n, words = prm.na * prm.nb, {}
        for pre in (False, True, None):  # None: back to the default
            vm.grid_set_mode(pre)
            for how in ("dev", "host"):
                _eq(_grid(vm, prm, how), want(vs, prm), (vs, pre, how))
            ws = torch.full((4 * n,), -1, dtype=torch.int64, device="cuda")
            cls = torch.zeros(n, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            vm.grid(_api_params(prm), workspace_ptr=ws.data_ptr(), cls_ptr=cls.data_ptr())
            vm.ctx.sync()
            words[pre] = ws.cpu().numpy().tobytes()
        assert words[False] == words[True] == words[None]  # the workspace too
        vm.close()


@pytest.mark.gpu
def test_other_orientations_and_grid_shapes(ctx):
    vs, lg, _ = MID
    vm = _filled(ctx, vs, lg)
    for name, prm in {**ORIENTATIONS, **SHAPES}.items():
        for how in ("dev", "host"):
            _eq(_grid(vm, prm, how), want(vs, prm), (name, how))
    wide = G.street_params(5)._replace(up_lo=-np.inf, up_hi=np.inf)
    _eq(_grid(vm, wide), want(vs, wide), "infinite band")
    far = G.street_params(5)._replace(origin_a=1e300, origin_b=-1e300)
    _eq(_grid(vm, far), want(vs, far), "far away")
    vm.close()


@pytest.mark.gpu
def test_grid_after_a_carve_and_after_a_removal(ctx):
    # a carve: the restatement on the downloaded table, whose carved slots keep their keys and count 0
    (pts, _, _, db), t, A2W, W2B = _carve_scene()
    from test_voxel_carve import _cam
    _fits(t.keys, CARVE_LG)
    vm = _map(ctx, CARVE_VS, CARVE_LG)
    _insert(vm, pts, A2W)
    before = _grid(vm, CARVE_PARAMS)
    _eq(before, G.grid_np(t, CARVE_PARAMS, CARVE_VS), "before the carve")
    assert vm.carve_host(db, _cam(), w2c12=W2B)["n_carved"] >= 50
    down = V.Table(*_stored(vm), 0, 0)
    dead = int(((down.ci >> np.uint64(40)) == 0).sum())
    assert dead >= 50 and np.array_equal(down.keys, t.keys)
    w = G.grid_np(down, CARVE_PARAMS, CARVE_VS)
    assert w.counts[0] == len(t.keys) - dead and not G.same(w, G.grid_np(t, CARVE_PARAMS, CARVE_VS))  # zero-count keys contribute nothing
    for how in ("dev", "host"):
        _eq(_grid(vm, CARVE_PARAMS, how), w, ("after the carve", how))
    vm.close()
    # a removal: the box and the road around it taken back out of the street
    vs, lg, cv = MID
    prm = G.street_params(cv)
    vm = _filled(ctx, vs, lg)
    gone = street()[_box_region(street())].copy()
    assert len(gone) >= 500
    dev = _dev(gone)
    c = vm.remove_host_counts(dev.data_ptr(), len(gone), m12=IDENT)
    assert c["n_removed"] == len(gone) and c["n_short"] == 0
    down = V.Table(*_stored(vm), 0, 0)
    assert np.array_equal(down.keys, table(vs).keys) and int(((down.ci >> np.uint64(40)) == 0).sum()) >= 100
    w = G.grid_np(down, prm, vs)
    assert G.same(w, G.grid_np(V.insert_np(street()[~_box_region(street())], IDENT, vs), prm, vs))  # as if never inserted
    box = sorted(G.street_cells(prm, vs)["box"])
    assert all(w.cls[at] == G.UNKNOWN and want(vs, prm).cls[at] == G.OBSTACLE for at in box)
    for how in ("dev", "host"):
        _eq(_grid(vm, prm, how), w, ("after the removal", how))
    vm.close()


@pytest.mark.gpu
def test_constructed_voxels_in_a_table_shorter_than_one_tile(ctx):
    vm = _map(ctx, G.CONSTRUCTED_VS, 8)  # 256 slots: one workgroup walks 2,048
    for i, (name, (p, prm, facts)) in enumerate(sorted(G.constructed().items())):
        t = V.insert_np(p, IDENT, G.CONSTRUCTED_VS)
        w = G.grid_np(t, prm, G.CONSTRUCTED_VS)
        assert w.counts[:3] == facts["counts"], name
        vm.clear()
        _insert(vm, p, IDENT)
        vm.grid_set_mode(i % 4 < 2)
        _eq(_grid(vm, prm, ("dev", "host")[i % 2]), w, name)
        _eq(_grid(vm, prm, ("host", "dev")[i % 2]), w, name)
    vm.grid_set_mode()
    # the street's grid from a short table too: its first 60 records
    few = street()[:60].copy()
    vm.clear()
    _insert(vm, few, IDENT)
    prm = G.street_params(2)
    w = G.grid_np(V.insert_np(few, IDENT, G.CONSTRUCTED_VS), prm, G.CONSTRUCTED_VS)
    assert w.counts[2] >= 1
    _eq(_grid(vm, prm), w, "short table")
    vm.close()


@pytest.mark.gpu
def test_bad_calls_launch_nothing_and_leave_the_map_usable(ctx):
    import torch
    from stereo_vo_amd import api
    L = ctx.L
    vs, lg, cv = G.STREET_SIZES[2]
    vm = _filled(ctx, vs, lg)
    good = G.street_params(cv)
    n = good.na * good.nb
    ws = torch.zeros(4 * n + 1, dtype=torch.int64, device="cuda")
    cls = torch.full((n,), 0xAA, dtype=torch.uint8, device="cuda")
    f32 = torch.full((n + 1,), 0x5555AAAA, dtype=torch.int32, device="cuda")
    u64 = torch.full((n + 1,), 0x6666666666666666, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    O = api.VoxelGridOut
    nan, inf = float("nan"), float("inf")

    def dev(prm=good, ws_ptr=ws.data_ptr(), out=None, counts=None, null_prm=False, null_out=False):
        o = out if out is not None else O(cls.data_ptr())
        p = _api_params(prm)
        return L.svo_voxel_map_grid_dev(vm.h, None if null_prm else C.byref(p), ws_ptr, None if null_out else C.byref(o), counts)

    r = good._replace
    host_cls = np.full((good.na, good.nb), 0xAA, np.uint8)
    calls = [(lambda: dev(null_prm=True), "null params"), (lambda: dev(ws_ptr=None), "null workspace"), (lambda: dev(null_out=True), "null out"),
             (lambda: dev(out=O(None)), "null cls"),
             (lambda: dev(r(up_axis=-1)), "up_axis"), (lambda: dev(r(up_axis=3)), "up_axis"), (lambda: dev(r(up_sign=0)), "up_sign"), (lambda: dev(r(up_sign=2)), "up_sign"),
             (lambda: dev(r(origin_a=nan)), "origin_a"), (lambda: dev(r(origin_a=inf)), "origin_a"), (lambda: dev(r(origin_b=nan)), "origin_b"),
             (lambda: dev(r(origin_b=-inf)), "origin_b"), (lambda: dev(r(cell_voxels=0)), "cell_voxels"), (lambda: dev(r(cell_voxels=1025)), "cell_voxels"),
             (lambda: dev(r(na=0)), "na outside"), (lambda: dev(r(na=8193)), "na outside"), (lambda: dev(r(nb=0)), "nb outside"), (lambda: dev(r(nb=8193)), "nb outside"),
             (lambda: dev(r(na=8192, nb=2049)), "na * nb"), (lambda: dev(r(up_lo=nan)), "NaN"), (lambda: dev(r(up_hi=nan)), "NaN"),
             (lambda: dev(r(up_lo=2.5, up_hi=2.0)), "up_lo above"), (lambda: dev(r(obstacle_step=-0.1)), "obstacle_step"),
             (lambda: dev(r(obstacle_step=nan)), "obstacle_step"), (lambda: dev(r(min_count=0)), "min_count"),
             (lambda: dev(ws_ptr=ws.data_ptr() + 4), "workspace must be 8-byte"), (lambda: dev(counts=u64.data_ptr() + 4), "counts must be 8-byte"),
             (lambda: dev(out=O(cls.data_ptr(), f32.data_ptr() + 2)), "top must be 4-byte"),
             (lambda: dev(out=O(cls.data_ptr(), None, f32.data_ptr() + 1)), "bottom must be 4-byte"),
             (lambda: dev(out=O(cls.data_ptr(), None, None, None, f32.data_ptr() + 2)), "n_voxels must be 4-byte"),
             (lambda: dev(out=O(cls.data_ptr(), None, None, None, None, u64.data_ptr() + 4)), "n_points must be 8-byte"),
             (lambda: L.svo_voxel_map_grid(vm.h, C.byref(_api_params(r(min_count=0))), C.byref(O(host_cls.ctypes.data)), None), "min_count"),
             (lambda: L.svo_voxel_map_grid(vm.h, C.byref(_api_params(good)), C.byref(O(None)), None), "null cls"),
             (lambda: L.svo_voxel_map_grid(vm.h, C.byref(_api_params(good)), None, None), "null out")]
    ctx.profile_select("voxel_grid")
    for call, word in calls:
        assert call() == -1 and word in L.svo_last_error(ctx.h).decode(), (word, L.svo_last_error(ctx.h).decode())
    assert ctx.profile_read()[1] == 0
    assert (cls.cpu().numpy() == 0xAA).all() and (f32.cpu().numpy() == 0x5555AAAA).all() and (u64.cpu().numpy() == 0x6666666666666666).all()
    assert (host_cls == 0xAA).all() and not ws.cpu().numpy().any()
    # the boundaries' accepted sides: the largest grid's shape limits, infinite bounds, a step of 0, one cell
    assert dev(good._replace(na=1, nb=1, up_lo=-inf, up_hi=inf, obstacle_step=0.0, cell_voxels=1024)) == 0
    assert ctx.profile_read()[1] == 1
    ctx.profile_select(None)
    with pytest.raises(api.SvoError):
        vm.grid(_api_params(good), cls_ptr=cls.data_ptr())  # no workspace
    with pytest.raises(api.SvoError):
        vm.grid_host(na=0)
    # the map is what it was, and gives its grid
    t = table(vs)
    got = _stored(vm)
    assert all(np.array_equal(g, getattr(t, k)) for g, k in zip(got, ("keys", "ci", "sx", "sy", "sz")))
    _eq(_grid(vm, good), want(vs, good))
    _eq(_grid(vm, good, "host"), want(vs, good))
    vm.close()
