"""The ground plan surface (include/svo.h, "Ground plan surface") against its restatement tests/grid_surface_ref.py, with == on
cls_out, support and the six counts, and on step and relief as bit patterns.

CPU: the restatement's two routes agree on every case used below (cell by cell over the whole grid where that is at most 400,000
footprint visits, over the corners, the edges' middles and 60 seeded cells otherwise); the random cases reach every outcome and every
rule alone; the constructed grids are what they were built to be; each deliberate misreading of the contract changes a stated case by
a stated count; the pure entries and the refusals that need no context; stereo_vo_amd/host/surface_args.h walked by
tests/sanitize/grid_surface_args_test.cpp under ASan + UBSan.
GPU: seeded random grids of ten shapes (the issue's seven, and 8 x 32, 9 x 33 and 5 x 65: the kept tile of 8 x 32 and one past its
edges, one past 4 x 64's) at r2 = 0, 1, 2, 8, 25 and 225; 8192 x 129, which has more tiles than a launch has workgroups, so that
workgroups take one tile or two, at r2 = 2 and 8; cliffs exactly on the seams of every tile shape in both directions; each
optional output left out alone, no counts; a repeated call; each rule switched off; the constructed grids through both entries; bad
calls.  Every device call runs into sentinel-filled outputs whose guard elements stay, cls and top between guard elements that would
be ground a thousand units up.

Misreadings, cells that change on the restatement ("random": random_case(63, 65) at r2 = 25, max_step 0.3, max_relief 0.6,
min_support_256 200, whose counts are 3,455 ground, 114 STEP, 328 ROUGH, 729 UNSUPPORTED, 83 NONFINITE, 2,284 kept):
  eight neighbours for the step 38 cls_out and 3,261 step (random); dstep >= max_step 2 cls_out ("0.3f against (double)0.3f");
  drelief >= max_relief 2 cls_out ("relief at the bound"); a square footprint 601 cls_out, 3,422 relief, 4,095 support (random);
  heights of cells that are not GROUND 3,060 cls_out, 813 step, 3,347 relief (random) and 2 cls_out ("across_an_obstacle"); offsets
  outside the grid as support 523 cls_out, 1,180 support (random); ROUGH before STEP 105 cls_out (random); the subtraction in f32 2
  cls_out ("big_f32_wrong"); a NONFINITE cell passed through 83 cls_out (random).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import grid_surface_ref as G
from test_host_sanitizers import _run_sanitized

FIELDS = ("cls_out", "step", "relief", "support")
RANDOM = (63, 65, 25)
MISREADINGS = {"step8": ("random", {"cls_out": 38, "step": 3261}), "step_ge": ("0.3f against (double)0.3f", {"cls_out": 2}),
               "relief_ge": ("relief at the bound", {"cls_out": 2}), "square": ("random", {"cls_out": 601, "relief": 3422, "support": 4095}),
               "nonground_heights": ("random", {"cls_out": 3060, "step": 813, "relief": 3347}), "outside_support": ("random", {"cls_out": 523, "support": 1180}),
               "rough_first": ("random", {"cls_out": 105}), "f32_sub": ("big_f32_wrong", {"cls_out": 2}), "nonfinite_through": ("random", {"cls_out": 83})}
GPU_SIZES = G.SIZES + ((8, 32), (9, 33), (5, 65))
OUTPUTS = ("step", "relief", "support")
MANY_TILES = (8192, 129)  # 5,120 tiles of 8 x 32, 4,608 of 16 x 16, 6,144 of 4 x 64: more than the 4,096 workgroups of a launch, and no multiple of them
PY_WHOLE = 400000  # footprint visits up to which the cell-by-cell route walks the whole grid


@functools.lru_cache(maxsize=None)
def case(na, nb):
    cls, top = G.random_case(na, nb)
    cls.setflags(write=False)
    top.setflags(write=False)
    return cls, top


@functools.lru_cache(maxsize=None)
def want(na, nb, r2):
    cls, top = case(na, nb)
    w, rules = G.surface_np(cls, top, G.random_params(cls, r2), detail=True)
    for a in w[:4]:
        a.setflags(write=False)
    return w, rules


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _diff(x, y):
    return {f: n for f in FIELDS for n in [int((_bits(getattr(x, f)) != _bits(getattr(y, f))).sum())] if n}


def _py_agrees(cls, top, prm, w):
    if prm.na * prm.nb * G.cells_of(G.r2_of(prm)) <= PY_WHOLE:
        return G.same(w, G.as_surface(G.surface_py(cls, top, prm), prm))
    return G.agrees_at(w, G.surface_py(cls, top, prm, G.sample_cells(prm.na, prm.nb, 60)))


# ===================================================================================================== CPU
def test_the_two_routes_of_the_restatement_agree_on_every_case():
    for na, nb in GPU_SIZES:
        cls, top = case(na, nb)
        for r2 in G.R2S:
            w, _ = want(na, nb, r2)
            assert _py_agrees(cls, top, G.random_params(cls, r2), w), (na, nb, r2)
            c = w.counts
            assert c[1] + c[2] + c[3] + c[5] == c[0] and c[0] + c[4] <= na * nb
    cls, top = G.seam_case()
    for r2 in (0, 2, 25):
        prm = G.params(cls, r2)
        assert _py_agrees(cls, top, prm, G.surface_np(cls, top, prm)), r2
    cls, top = case(*MANY_TILES)
    for r2 in (2, 8):
        assert _py_agrees(cls, top, G.random_params(cls, r2), want(*MANY_TILES, r2)[0]), r2
    for name, (cls, top, prm) in G.constructed().items():
        assert G.same(G.surface_np(cls, top, prm), G.as_surface(G.surface_py(cls, top, prm), prm)), name


def test_the_random_cases_reach_every_outcome_and_every_rule_alone():
    """Conditions on the inputs: each of STEP, ROUGH, UNSUPPORTED, NONFINITE and kept occurs, and cells exist that rule 6a, 6b or 6c
    decides alone (the other two conditions false), in one case at least, and all of it together in the misreadings' case."""
    seen = np.zeros(5, bool)
    alone = np.zeros(3, bool)
    for na, nb in GPU_SIZES:
        for r2 in G.R2S:
            w, (a, b, c) = want(na, nb, r2)
            seen |= np.array([w.counts[k] > 0 for k in (1, 2, 3, 4, 5)])
            alone |= np.array([(a & ~b & ~c).any(), (b & ~a & ~c).any(), (c & ~a & ~b).any()])
    assert seen.all() and alone.all(), (seen, alone)
    w, (a, b, c) = want(*RANDOM)
    assert w.counts == (3455, 114, 328, 729, 83, 2284)
    assert int((a & ~b & ~c).sum()) > 0 and int((b & ~a & ~c).sum()) > 0 and int((c & ~a & ~b).sum()) > 0
    assert (a & b).any() and (b & c).any()  # and cells where the order of the rules decides
    cls, top = case(*RANDOM[:2])
    assert (cls >= 32).sum() > 0 and np.isnan(top).any() and np.isposinf(top).any() and (np.isneginf(top) & (cls == 1)).any()
    # at r2 = 0 the footprint is the cell: relief 0, support 0 or 1
    w, _ = want(63, 65, 0)
    assert w.counts[2] == 0 and set(np.unique(w.support)) == {0, 1} and (w.relief[w.relief >= 0] == 0).all()
    assert np.array_equal(w.support == 1, w.step >= 0)


def test_the_constructed_grids_are_what_they_were_built_to_be():
    g = G.constructed()
    S = lambda name: G.surface_np(*g[name])
    # the terrace: STEP along the ledge and along the ramp's sides, the ramp's lane keeps its class from plateau to plateau
    t = G.TERRACE
    s = S("terrace")
    ledge = t["ledge"]
    outside_ramp = [ia for ia in range(t["na"]) if not t["ramp_rows"][0] <= ia < t["ramp_rows"][1]]
    assert (s.cls_out[outside_ramp, ledge - 1:ledge + 1] == G.STEP).all() and (s.step[outside_ramp, ledge - 1:ledge + 1] == 1.0).all()
    lane = slice(*t["lane_rows"])
    assert (s.cls_out[lane, :] == 1).all() and s.step[lane, :].max() <= np.float32(0.1) + 1e-6
    for inner, outer in ((t["ramp_rows"][0], t["ramp_rows"][0] - 1), (t["ramp_rows"][1] - 1, t["ramp_rows"][1])):  # the ramp's two sides
        d = np.abs(g["terrace"][1][inner].astype(np.float64) - g["terrace"][1][outer].astype(np.float64))
        assert np.array_equal(s.cls_out[inner] == G.STEP, d > t["max_step"]) and np.array_equal(s.cls_out[outer] == G.STEP, d > t["max_step"])
        assert (d > t["max_step"]).sum() == 3
    assert s.counts == (240, 24, 0, 0, 0, 216)
    # without the ramp the ledge is closed from edge to edge
    cls, _, prm = g["terrace"]
    closed = G.surface_np(cls, G.terrace_tops(ramp=False), prm)
    assert (closed.cls_out[:, ledge - 1:ledge + 1] == G.STEP).all() and closed.counts[1] == 2 * t["na"]
    # the slope: no step anywhere, rough everywhere, the corner cells included
    s = S("slope")
    assert s.counts == (360, 0, 360, 0, 0, 0) and (s.step <= 0.25).all() and s.relief.min() == 1.25 and s.relief.max() == 2.5
    # strictness at the step, with the f32 -> f64 conversion of 0.3f
    assert G.F03 > 0.3
    assert S("0.3f against (double)0.3f").cls_out.tolist() == [[1, 1]] and S("0.3f against 0.3").cls_out.tolist() == [[G.STEP, G.STEP]]
    assert S("relief at the bound").cls_out.tolist() == [[1, 1]] and S("relief at the bound").relief.tolist() == [[0.5, 0.5]]
    # -0.0f beside +0.0f: no step, no relief, and both zeros are +0.0
    s = S("zeros")
    assert s.cls_out.tolist() == [[1, 1]] and s.step.view(np.uint32).tolist() == [[0, 0]] and s.relief.view(np.uint32).tolist() == [[0, 0]]
    # 2^24 and 1: 16777215 either way; 2^24 and -1: 16777217 in f64, 16777216 in f32
    s = S("big_exact")
    assert s.step.tolist() == [[16777215.0] * 2] and np.float32(16777216.0) - np.float32(1.0) == np.float32(16777215.0)
    assert not _diff(s, G.surface_np(*g["big_exact"], variant="f32_sub"))
    assert S("big_f32_wrong").cls_out.tolist() == [[G.STEP] * 2] and np.float32(16777216.0) - np.float32(-1.0) == np.float32(16777216.0)
    assert G.surface_np(*g["big_f32_wrong"], variant="f32_sub").cls_out.tolist() == [[1, 1]]
    # the island: 1 of 9 cells, 256 < 128 * 9
    s = S("island")
    assert s.cls_out[1, 1] == G.UNSUPPORTED and (s.support == 1).all() and s.counts == (1, 0, 0, 1, 0, 0)
    assert (np.delete(s.cls_out.ravel(), 4) == 0).all()
    # the obstacle between two heights is no ground: no step
    s = S("across_an_obstacle")
    assert s.cls_out.tolist() == [[1, 2, 1]] and s.step.tolist() == [[0.0, -1.0, 0.0]] and s.support.tolist() == [[1, 0, 1]]


def test_every_misreading_of_the_contract_changes_a_stated_case_by_a_stated_count():
    cls, top = case(*RANDOM[:2])
    cases = {"random": (cls, top, G.random_params(cls, RANDOM[2])), **G.constructed()}
    got = {}
    for variant, (name, _) in MISREADINGS.items():
        cls, top, prm = cases[name]
        got[variant] = (name, _diff(G.surface_np(cls, top, prm), G.surface_np(cls, top, prm, variant=variant)))
        assert got[variant][1], variant
    assert got == MISREADINGS, got
    assert _diff(G.surface_np(*cases["across_an_obstacle"]), G.surface_np(*cases["across_an_obstacle"], variant="nonground_heights")) == {"cls_out": 2, "step": 2}
    assert set(MISREADINGS) == set(G.VARIANTS)


def _api_params(prm):
    from stereo_vo_amd import api
    return api.GridSurfaceParams(*prm)


def test_pure_entries_and_refusals_without_a_context():
    from stereo_vo_amd import api
    L = api.lib()
    g = api.voxel_grid_default_params(0.1)
    d = api.grid_surface_default_params(g, 0.1)
    assert (d.na, d.nb, d.ground_mask, d.max_step, d.max_relief, d.min_support_256) == (256, 256, 1 << api.VOXEL_GRID_LEVEL, 0.3, 0.6, 0)
    assert d.cell_size == 5.0 * float(np.float32(0.1)) and d.footprint_radius == 1.5 * d.cell_size
    assert G.r2_of(G.Params(*(getattr(d, f) for f, _ in d._fields_))) == 2
    g.na, g.nb, g.cell_voxels, g.obstacle_step = 17, 300, 3, 0.25
    d = api.grid_surface_default_params(g, 0.25)
    assert (d.na, d.nb, d.cell_size, d.max_step, d.footprint_radius, d.max_relief) == (17, 300, 0.75, 0.25, 1.125, 0.5)
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(api.SvoError):
            api.grid_surface_default_params(g, bad)
    for field, value in (("na", 0), ("nb", 8193), ("cell_voxels", 0), ("obstacle_step", float("nan")), ("obstacle_step", -1.0)):
        h = api.voxel_grid_default_params(0.1)
        setattr(h, field, value)
        with pytest.raises(api.SvoError):
            api.grid_surface_default_params(h, 0.1)
    assert L.svo_grid_surface_default_params(None, C.c_float(0.1), C.byref(d)) == -1
    assert L.svo_grid_surface_default_params(C.byref(g), C.c_float(0.1), None) == -1
    # D(r2)
    assert [api.grid_surface_footprint_cells(r2) for r2 in (0, 1, 2, 4, 8, 25, 225)] == [1, 5, 9, 13, 25, 81, 709]
    assert all(api.grid_surface_footprint_cells(r2) == G.cells_of(r2) for r2 in range(226))
    assert api.grid_surface_footprint_cells(226) == 0 and api.grid_surface_footprint_cells(0xFFFFFFFF) == 0
    assert [G.half_widths(r2) for r2 in (0, 1, 2)] == [[0], [0, 1, 0], [1, 1, 1]] and sum(2 * w + 1 for w in G.half_widths(225)) == 709
    assert (api.GRID_SURFACE_STEP, api.GRID_SURFACE_ROUGH, api.GRID_SURFACE_UNSUPPORTED, api.GRID_SURFACE_SOURCES) == (G.STEP, G.ROUGH, G.UNSUPPORTED, G.SOURCES) == (3, 4, 5, 0x3C)
    assert api.GRID_SURFACE_COUNTS == G.COUNTS
    # a null context is refused by both entries before anything else is looked at
    buf = (C.c_double * 12)()
    out = api.GridSurfaceOut(C.addressof(buf) + 32)
    assert L.svo_grid_surface_dev(None, buf, buf, C.byref(d), C.byref(out), None) == -1
    assert L.svo_grid_surface(None, buf, buf, C.byref(d), C.byref(out), None) == -1
    assert L.svo_grid_surface_dev(None, None, None, None, None, None) == -1 and L.svo_grid_surface(None, None, None, None, None, None) == -1


def test_grid_surface_args_every_refusal_the_footprint_table_and_the_defaults(tmp_path):
    """host/surface_args.h on the CPU under ASan + UBSan: every refusal at its boundary with code and exact message, the order of the
    refusals, rc * rc at 226, r2, the half-width table for r2 = 0, 1, 2, 8, 225 and every r2 against a brute-force count, D, the
    support comparison's edges, the tile and the defaults."""
    _run_sanitized(tmp_path, "grid_surface_args_test", "grid surface args ok")


# ===================================================================================================== GPU
_SENT = {"cls_out": (np.uint8, 0xBB), "step": (np.int32, 0x77777777), "relief": (np.int32, 0x5555AAAA), "support": (np.int16, 0x3333)}
_KIND = {"cls_out": np.uint8, "step": np.float32, "relief": np.float32, "support": np.uint16}


def _run(ctx, cls, top, prm, how="dev", skip=(), counts=True, keep=None):
    """One surface by the named entry, as a G.Surface (None for an output in `skip`, and for counts when they are left out).  The device
    entry runs into sentinel-filled outputs, one guard element before and behind each; cls and top stand between guard elements that
    would be LEVEL ground 1,000 up.  keep: a dict that receives the raw bytes of every output."""
    import torch
    p = _api_params(prm)
    if how == "host":
        *arrays, c = ctx.grid_surface_host(cls, top, p)
        return G.Surface(*arrays, tuple(c[k] for k in G.COUNTS))
    n = prm.na * prm.nb
    d_cls = torch.full((n + 2,), 1, dtype=torch.uint8, device="cuda")
    d_cls[1:-1] = torch.from_numpy(np.array(cls).ravel()).cuda()
    d_top = torch.full((n + 2,), 1000.0, dtype=torch.float32, device="cuda")
    d_top[1:-1] = torch.from_numpy(np.array(top).ravel()).cuda()
    bufs = {k: torch.full((n + 2,), v, dtype=getattr(torch, np.dtype(t).name), device="cuda") for k, (t, v) in _SENT.items()}
    cnt = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ptr = {k: None if k in skip else b.data_ptr() + b.element_size() for k, b in bufs.items()}
    out = ctx.grid_surface(d_cls.data_ptr() + 1, d_top.data_ptr() + 4, p, counts_ptr=cnt.data_ptr() + 8 if counts else None,
                           **{k + "_ptr": v for k, v in ptr.items()})
    assert out["cls_out"] == ptr["cls_out"] and (out["na"], out["nb"]) == (prm.na, prm.nb)
    ctx.sync()  # the tensors go out of scope behind the return
    assert np.array_equal(d_cls.cpu().numpy()[1:-1].reshape(cls.shape), cls)  # only read
    assert np.array_equal(d_top.cpu().numpy()[1:-1].view(np.uint32).reshape(top.shape), np.asarray(top).view(np.uint32))
    got = {}
    for k, (t, v) in _SENT.items():
        a = bufs[k].cpu().numpy()
        assert a[0] == v and a[-1] == v, k  # nothing beside the outputs is written
        if k in skip:
            assert (a == v).all(), k
            got[k] = None
        else:
            got[k] = a[1:-1].view(_KIND[k]).reshape(prm.na, prm.nb)
        if keep is not None:
            keep[k] = a.tobytes()
    c = cnt.cpu().numpy()
    assert c[0] == c[-1] == -1 and (counts or (c == -1).all())
    return G.Surface(got["cls_out"], got["step"], got["relief"], got["support"], tuple(int(v) for v in c[1:7]) if counts else None)


def _eq(got, w, what=""):
    for name in FIELDS:
        if getattr(got, name) is not None:
            x, y = _bits(getattr(got, name)), _bits(getattr(w, name))
            assert np.array_equal(x, y), (what, name, int((x != y).sum()), np.argwhere(x != y)[:5].tolist())
    if got.counts is not None:
        assert tuple(got.counts) == tuple(w.counts), (what, got.counts, w.counts)


@pytest.mark.gpu
@pytest.mark.parametrize("na,nb", GPU_SIZES)
def test_random_grids(ctx, na, nb):
    cls, top = case(na, nb)
    for r2 in G.R2S:
        w, _ = want(na, nb, r2)
        got = _run(ctx, cls, top, G.random_params(cls, r2))
        print(na, nb, r2, "counts", got.counts)
        _eq(got, w, r2)


@pytest.mark.gpu
def test_a_grid_of_more_tiles_than_a_launch_has_workgroups(ctx):
    na, nb = MANY_TILES
    assert -(-na // 8) * -(-nb // 32) > 4096 and -(-na // 16) * -(-nb // 16) > 4096 and -(-na // 4) * -(-nb // 64) > 4096
    cls, top = case(na, nb)
    for r2 in (2, 8):
        w, _ = want(na, nb, r2)
        assert all(c > 0 for c in w.counts)
        got = _run(ctx, cls, top, G.random_params(cls, r2))
        print(na, nb, r2, "counts", got.counts)
        _eq(got, w, r2)


@pytest.mark.gpu
def test_cliffs_exactly_on_the_tile_seams_in_both_directions(ctx):
    cls, top = G.seam_case()
    for r2 in (0, 2, 25):
        prm = G.params(cls, r2)
        w = G.surface_np(cls, top, prm)
        # both cells of every seam are STEP, over the seam's whole length, and nothing else is
        steps = np.zeros(cls.shape, bool)
        for k in (8, 16, 32):
            steps[k - 1:k + 1, :] = True
        for k in (16, 32, 64):
            steps[:, k - 1:k + 1] = True
        assert np.array_equal(w.cls_out == G.STEP, steps) and w.counts[1] == int(steps.sum())
        assert (r2 == 25) == (w.counts[2] > 0)  # only the widest of the three reaches from a cell that is no STEP across a cliff
        for how in ("dev", "host"):
            _eq(_run(ctx, cls, top, prm, how), w, (r2, how))


@pytest.mark.gpu
def test_optional_outputs_no_counts_the_host_entry_and_a_repeated_call(ctx):
    from stereo_vo_amd import api
    na, nb, r2 = 63, 65, 8
    cls, top = case(na, nb)
    prm = G.random_params(cls, r2)
    w, _ = want(na, nb, r2)
    for skip in [(k,) for k in OUTPUTS] + [OUTPUTS]:
        got = _run(ctx, cls, top, prm, skip=skip)
        assert all(getattr(got, k) is None for k in skip) and got.cls_out is not None
        _eq(got, w, skip)
    _eq(_run(ctx, cls, top, prm, counts=False), w, "no counts")
    _eq(_run(ctx, cls, top, prm, skip=OUTPUTS, counts=False), w, "cls_out alone")
    # the host entry: everything, then cls_out alone with no counts
    _eq(_run(ctx, cls, top, prm, "host"), w, "host")
    out = np.full((na, nb), 0xBB, np.uint8)
    p = _api_params(prm)
    assert ctx.L.svo_grid_surface(ctx.h, cls.ctypes.data, top.ctypes.data, C.byref(p), C.byref(api.GridSurfaceOut(out.ctypes.data)), None) == 0
    assert np.array_equal(out, w.cls_out)
    # twice: the same bytes in every output
    first, second = {}, {}
    _eq(_run(ctx, cls, top, prm, keep=first), w)
    _eq(_run(ctx, cls, top, prm, keep=second), w)
    assert first == second and set(first) == set(FIELDS)


@pytest.mark.gpu
def test_each_rule_switched_off_by_its_parameter(ctx):
    na, nb, r2 = 63, 65, 8
    cls, top = case(na, nb)
    on = G.random_params(cls, r2)
    full = want(na, nb, r2)[0].counts
    assert full[1] > 0 and full[2] > 0 and full[3] > 0
    for off, gone in ((dict(max_step=G.INF), 1), (dict(max_relief=G.INF), 2), (dict(min_support_256=0), 3),
                      (dict(max_step=G.INF, max_relief=G.INF, min_support_256=0), None)):
        prm = on._replace(**off)
        w = G.surface_np(cls, top, prm)
        if gone is None:
            assert w.counts[1:4] == (0, 0, 0) and w.counts[5] == w.counts[0]
            assert np.array_equal(w.cls_out[w.step >= 0], cls[w.step >= 0])  # every GROUND cell keeps its class
        else:
            assert w.counts[gone] == 0 and all(w.counts[k] > 0 for k in (1, 2, 3) if k != gone)
        _eq(_run(ctx, cls, top, prm), w, off)
    # the other way round: every threshold at 0 and the whole footprint asked for
    prm = on._replace(max_step=0.0, max_relief=0.0, min_support_256=256)
    w = G.surface_np(cls, top, prm)
    assert w.counts[5] < full[5]
    _eq(_run(ctx, cls, top, prm), w, "all at their strictest")
    # another ground mask: OBSTACLE and UNKNOWN cells are the ground, LEVEL cells pass through
    prm = on._replace(ground_mask=1 << 0 | 1 << 2 | 1 << 31)
    w = G.surface_np(cls, top, prm)
    assert w.counts[0] > 0 and w.counts[4] > 0  # the UNKNOWN cells' tops are -inf: NONFINITE
    _eq(_run(ctx, cls, top, prm), w, "another mask")


@pytest.mark.gpu
def test_constructed_grids_through_both_entries(ctx):
    for name, (cls, top, prm) in G.constructed().items():
        w = G.surface_np(cls, top, prm)
        for how in ("dev", "host"):
            _eq(_run(ctx, cls, top, prm, how), w, (name, how))
    cls, _, prm = G.constructed()["terrace"]
    top = G.terrace_tops(ramp=False)
    _eq(_run(ctx, cls, top, prm), G.surface_np(cls, top, prm), "the terrace without its ramp")


@pytest.mark.gpu
def test_bad_calls_launch_nothing_and_leave_the_context_usable(ctx):
    import torch
    from stereo_vo_amd import api
    L = ctx.L
    na, nb, r2 = 33, 31, 2
    cls, top = case(na, nb)
    good = G.random_params(cls, r2)
    n = na * nb
    d_cls = torch.from_numpy(np.array(cls).ravel()).cuda()
    d_top = torch.from_numpy(np.array(top).ravel()).cuda()
    f32 = torch.full((2, n + 1), 0x5555AAAA, dtype=torch.int32, device="cuda")
    u16 = torch.full((n + 1,), 0x3333, dtype=torch.int16, device="cuda")
    u8 = torch.full((n + 1,), 0xBB, dtype=torch.uint8, device="cuda")
    u64 = torch.full((8,), 0x6666666666666666, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    O = api.GridSurfaceOut
    nan, inf = float("nan"), float("inf")
    outp, stepp, relp, supp = u8.data_ptr(), f32[0].data_ptr(), f32[1].data_ptr(), u16.data_ptr()

    def dev(prm=good, cls_ptr=d_cls.data_ptr(), top_ptr=d_top.data_ptr(), out=None, counts=None, null_prm=False, null_out=False):
        o = out if out is not None else O(outp, stepp, relp, supp)
        p = _api_params(prm)
        return L.svo_grid_surface_dev(ctx.h, cls_ptr, top_ptr, None if null_prm else C.byref(p), None if null_out else C.byref(o), counts)

    r = good._replace
    h_out = np.full((na, nb), 0xBB, np.uint8)
    host = lambda prm=good, c=cls.ctypes.data, t=top.ctypes.data, o=O(h_out.ctypes.data): L.svo_grid_surface(ctx.h, c, t, C.byref(_api_params(prm)), C.byref(o), None)
    calls = [(lambda: dev(cls_ptr=None), "null cls"), (lambda: dev(top_ptr=None), "null top"), (lambda: dev(null_prm=True), "null params"),
             (lambda: dev(null_out=True), "null out"), (lambda: dev(out=O(None, stepp)), "null cls_out"),
             (lambda: dev(out=O(d_cls.data_ptr())), "cls_out must not be cls"),
             (lambda: dev(r(na=0)), "na outside"), (lambda: dev(r(na=8193)), "na outside"), (lambda: dev(r(nb=0)), "nb outside"),
             (lambda: dev(r(nb=8193)), "nb outside"), (lambda: dev(r(na=8192, nb=2049)), "na * nb"), (lambda: dev(r(ground_mask=0)), "ground_mask"),
             (lambda: dev(r(cell_size=0.0)), "cell_size"), (lambda: dev(r(cell_size=-0.5)), "cell_size"), (lambda: dev(r(cell_size=nan)), "cell_size"),
             (lambda: dev(r(cell_size=inf)), "cell_size"), (lambda: dev(r(max_step=-0.1)), "max_step"), (lambda: dev(r(max_step=nan)), "max_step"),
             (lambda: dev(r(footprint_radius=-0.1)), "footprint_radius must be"), (lambda: dev(r(footprint_radius=nan)), "footprint_radius must be"),
             (lambda: dev(r(footprint_radius=inf)), "footprint_radius must be"), (lambda: dev(r(footprint_radius=8.0)), "beyond 15 cells"),
             (lambda: dev(r(footprint_radius=float(np.sqrt(226.0)) * 0.5 * (1 + 1e-15))), "beyond 15 cells"),
             (lambda: dev(r(max_relief=-0.1)), "max_relief"), (lambda: dev(r(max_relief=nan)), "max_relief"),
             (lambda: dev(r(min_support_256=-1)), "min_support_256"), (lambda: dev(r(min_support_256=257)), "min_support_256"),
             (lambda: dev(top_ptr=d_top.data_ptr() + 2), "top must be 4-byte"), (lambda: dev(out=O(outp, stepp + 2)), "step must be 4-byte"),
             (lambda: dev(out=O(outp, None, relp + 1)), "relief must be 4-byte"), (lambda: dev(out=O(outp, None, None, supp + 1)), "support must be 2-byte"),
             (lambda: dev(counts=u64.data_ptr() + 4), "counts must be 8-byte"),
             (lambda: host(c=None), "null cls"), (lambda: host(t=None), "null top"),
             (lambda: L.svo_grid_surface(ctx.h, cls.ctypes.data, top.ctypes.data, None, C.byref(O(h_out.ctypes.data)), None), "null params"),
             (lambda: L.svo_grid_surface(ctx.h, cls.ctypes.data, top.ctypes.data, C.byref(_api_params(good)), None, None), "null out"),
             (lambda: host(o=O(None)), "null cls_out"), (lambda: host(o=O(cls.ctypes.data)), "cls_out must not be cls"),
             (lambda: host(r(min_support_256=300)), "min_support_256"), (lambda: host(r(footprint_radius=7.6)), "beyond 15 cells")]
    ctx.profile_select("grid_surface")
    for call, word in calls:
        assert call() == -1 and word in L.svo_last_error(ctx.h).decode(), (word, L.svo_last_error(ctx.h).decode())
    assert ctx.profile_read()[1] == 0
    assert (f32.cpu().numpy() == 0x5555AAAA).all() and (u16.cpu().numpy() == 0x3333).all() and (u8.cpu().numpy() == 0xBB).all()
    assert (u64.cpu().numpy() == 0x6666666666666666).all() and (h_out == 0xBB).all()
    # the boundaries' accepted sides in one call: one cell, every mask bit, the widest footprint, both thresholds at +inf, all the support
    assert dev(good._replace(na=1, nb=1, ground_mask=0xFFFFFFFF, cell_size=1.0, footprint_radius=15.0, max_step=inf, max_relief=inf, min_support_256=256),
               out=O(outp, stepp + 4, relp + 4, supp + 2), counts=u64.data_ptr() + 8) == 0
    assert ctx.profile_read()[1] == 1
    ctx.profile_select(None)
    with pytest.raises(api.SvoError):
        ctx.grid_surface(d_cls.data_ptr(), d_top.data_ptr(), _api_params(good))  # no cls_out
    with pytest.raises(api.SvoError):
        ctx.grid_surface_host(cls, top, _api_params(good), min_support_256=257)
    with pytest.raises(ValueError):
        ctx.grid_surface_host(cls, top, _api_params(good._replace(na=5)))
    with pytest.raises(ValueError):
        ctx.grid_surface_host(cls, top[:, :5], _api_params(good))
    # the context is what it was, and gives the surface
    w, _ = want(na, nb, r2)
    _eq(_run(ctx, cls, top, good), w)
    _eq(_run(ctx, cls, top, good, "host"), w)
