"""The ground plan clearance (include/svo.h, "Ground plan clearance") against its restatement tests/grid_clearance_ref.py, with
== on dist2, nearest, blocked and the four counts, and on clearance as bit patterns.

CPU: the restatement's two routes agree on every grid used below; dist2 equals scipy's Euclidean distance transform where scipy is
there; the constructed grids are what they were built to be; each deliberate misreading of the contract changes a result; the pure
entries and the refusals that need no context; stereo_vo_amd/host/clearance_args.h walked by tests/sanitize/grid_clearance_args_test.cpp
under ASan + UBSan.
GPU: seeded random grids of nine shapes at max_dist 1, 5 and 64 and three densities; the constructed grids; every byte value under
four masks; the inflation at an integer square, just below it, at 0 and beyond the clamp; every optional output left out; the host
entry; a repeated call; bad calls.  Every device call runs into a dirty workspace and sentinel-filled outputs whose guard elements stay.

Misreadings, cells that change on the restatement (grid "sparse": 63 x 65, density 0.01, 26 sources, max_dist 5, inflate_radius 1.2 at
0.5 per cell; "values": every byte value once, 16 x 16, mask 1 << 0 | 1 << 2, max_dist 5):
  tie to the larger index 14 nearest (sparse); d2 < max_dist^2 194 dist2 (sparse); the square window without the disc 573 dist2
  (sparse); chessboard distance 1,711 dist2 (sparse); Manhattan distance 1,130 dist2 (sparse); the row searched to the left only 663
  dist2 (sparse); NONE for sources 26 dist2 (sparse); cls & 31 instead of cls < 32 105 dist2 and 14 blocked == 2 (values).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import grid_clearance_ref as G
from test_host_sanitizers import _run_sanitized

SPARSE = (63, 65, 0.01, 5)
MISREADINGS = {"tie_larger": ("sparse", "nearest", 14), "lt_max": ("sparse", "dist2", 194), "square": ("sparse", "dist2", 573),
               "chessboard": ("sparse", "dist2", 1711), "manhattan": ("sparse", "dist2", 1130), "row_left_only": ("sparse", "dist2", 663),
               "none_for_sources": ("sparse", "dist2", 26), "wrap32": ("values", "dist2", 105)}
VALUES_MD = 5
BELOW_1P5 = float(np.nextafter(1.5, 0.0))
# name -> (inflate_radius, R2) at 0.5 per cell and max_dist 5: rc * rc an integer, the double just below, nothing, the clamp
INFLATIONS = {"rc 3": (1.5, 9), "just below rc 3": (BELOW_1P5, 8), "0": (0.0, 0), "beyond the clamp": (1e6, 25), "overflow": (1.7e308, 25)}
OUTPUTS = ("nearest", "clearance", "blocked")


@functools.lru_cache(maxsize=None)
def want(na, nb, density, max_dist, inflate_radius=1.2):
    cls = G.random_grid(na, nb, density)
    w = G.clearance_np(cls, G.params(cls, max_dist, inflate_radius=inflate_radius))
    for a in w[:4]:
        a.setflags(write=False)
    return w


def _sparse():
    na, nb, density, md = SPARSE
    cls = G.random_grid(na, nb, density)
    return cls, G.params(cls, md, inflate_radius=1.2)


def _inflation_grid():
    cls = np.array(G.constructed()["disc"][0])
    cls[0, 0] = 2  # a second source, so that the inflation has two discs to fill
    return cls


# ===================================================================================================== CPU
def test_the_two_routes_of_the_restatement_agree_on_every_grid():
    for na, nb in G.SIZES:
        for density in G.DENSITIES:
            cls = G.random_grid(na, nb, density)
            for md in G.MAX_DISTS:
                a = want(na, nb, density, md)
                assert G.same(a, G.clearance_py(cls, G.params(cls, md, inflate_radius=1.2))), (na, nb, density, md)
                assert sum(a.counts[:3]) == na * nb and a.counts[0] == int((cls == 2).sum())
    # the shapes are what the kernels' paths need: grids with and without a source, reached and unreached cells, inflated cells
    assert want(1, 1, 0.002, 5).counts == (0, 0, 1, 0) and want(256, 256, 0.002, 5).counts[2] > 50000 and want(256, 256, 0.002, 64).counts[2] == 0
    c = want(130, 300, 0.05, 1).counts
    assert c[2] > 1000 and c[3] == c[1] > 1000  # rc = 2.4, R2 = 5 clamped to max_dist^2 = 1: every reached cell is inside the inflation
    assert want(130, 300, 0.05, 5).counts[3] > 10000
    cls, prm = _sparse()
    assert G.same(G.clearance_np(cls, prm), G.clearance_py(cls, prm))
    cls, masks = G.all_values()
    for mask in masks:
        prm = G.params(cls, VALUES_MD, source_mask=mask, inflate_radius=0.6)
        a = G.clearance_np(cls, prm)
        assert G.same(a, G.clearance_py(cls, prm)), hex(mask)
        assert a.counts[0] == bin(mask).count("1")  # each class below 32 stands once in the grid; 32 .. 255 are never sources
        assert [int(v) for v in np.flatnonzero(a.dist2.ravel() == 0)] == [c for c in range(32) if mask >> c & 1]
    cls = _inflation_grid()
    for name, (radius, r2) in INFLATIONS.items():
        prm = G.params(cls, 5, inflate_radius=radius)
        a = G.clearance_np(cls, prm)
        assert G.same(a, G.clearance_py(cls, prm)) and G.r2_of(prm) == r2, name
        assert a.counts[3] == int(((a.dist2 > 0) & (a.dist2 <= r2)).sum()), name
    got = {name: G.clearance_np(cls, G.params(cls, 5, inflate_radius=radius)).counts[3] for name, (radius, _) in INFLATIONS.items()}
    assert got["rc 3"] > got["just below rc 3"] > got["0"] == 0 and got["beyond the clamp"] == got["overflow"] > got["rc 3"], got


def test_the_constructed_grids_are_what_they_were_built_to_be():
    for name, (cls, prm, facts) in G.constructed().items():
        a = G.clearance_np(cls, prm)
        assert G.same(a, G.clearance_py(cls, prm)), name
        assert a.counts == facts["counts"], (name, a.counts)
        for at, fact in facts.items():
            if at != "counts":
                assert (int(a.dist2[at]), int(a.nearest[at])) == fact, (name, at, int(a.dist2[at]), int(a.nearest[at]))
    a = G.clearance_np(*G.constructed()["disc"][:2])
    assert a.clearance[9, 10] == np.float32(2.5) and a.clearance[6, 6] == 0.0 and np.isinf(a.clearance[10, 10]) and a.clearance[7, 7] == np.float32(np.sqrt(2.0) * 0.5)
    a = G.clearance_np(*G.constructed()["all_sources"][:2])
    assert (a.blocked == 2).all() and (a.nearest.ravel() == np.arange(63)).all()
    # the case of the strict stop: the own row's source is met first and is not the answer
    cls, prm, _ = G.constructed()["earlier_row_tie"]
    assert cls[4, 6] == 2 and cls[1, 3] == 2 and int(G.clearance_np(cls, prm).nearest[4, 3]) == 1 * 7 + 3


def test_dist2_is_the_euclidean_distance_transform_where_nothing_is_capped():
    ndi = pytest.importorskip("scipy.ndimage")
    cases = [(G.random_grid(na, nb, density), 128) for na, nb in ((63, 65), (50, 41), (1, 257)) for density in (0.002, 0.05, 0.5)]
    cases += [(c, 64) for c, _, _ in (G.constructed()[k] for k in ("corners", "four_way_tie", "row_tie", "earlier_row_tie"))]
    done = 0
    for cls, md in cases:
        src = G.sources_np(cls, 1 << 2)
        if not src.any():
            continue
        a = G.clearance_np(cls, G.params(cls, md))
        edt2 = np.rint(ndi.distance_transform_edt(~src) ** 2)
        edt2[edt2 > md * md] = G.NONE  # only the 1 x 257 grids are longer than 128
        assert np.array_equal(a.dist2.astype(np.float64), edt2), cls.shape
        done += 1
    assert done >= 10


def test_every_misreading_of_the_contract_changes_a_result():
    cls_s, prm_s = _sparse()
    cls_v, masks = G.all_values()
    grids = {"sparse": (cls_s, prm_s), "values": (cls_v, G.params(cls_v, VALUES_MD, source_mask=masks[1], inflate_radius=0.6))}
    assert int(G.sources_np(cls_s, prm_s.source_mask).sum()) == 26
    got = {}
    for variant, (grid, field, _) in MISREADINGS.items():
        cls, prm = grids[grid]
        right, wrong = G.clearance_np(cls, prm), G.clearance_np(cls, prm, variant=variant)
        got[variant] = (grid, field, int((getattr(right, field) != getattr(wrong, field)).sum()))
        assert got[variant][2] > 0, variant
    assert got == MISREADINGS, got
    cls, prm = grids["values"]
    assert int(((G.clearance_np(cls, prm, variant="wrap32").blocked == 2) != (G.clearance_np(cls, prm).blocked == 2)).sum()) == 14
    assert set(MISREADINGS) == set(G.VARIANTS)


def _api_params(prm):
    from stereo_vo_amd import api
    return api.GridClearanceParams(*prm)


def test_pure_entries_and_refusals_without_a_context():
    from stereo_vo_amd import api
    L = api.lib()
    g = api.voxel_grid_default_params(0.1)
    d = api.grid_clearance_default_params(g, 0.1)
    assert (d.na, d.nb, d.source_mask, d.max_dist, d.inflate_radius) == (256, 256, 1 << api.VOXEL_GRID_OBSTACLE, 64, 0.0)
    assert d.cell_size == 5.0 * float(np.float32(0.1))
    g.na, g.nb, g.cell_voxels = 17, 300, 3
    d = api.grid_clearance_default_params(g, 0.25)
    assert (d.na, d.nb, d.cell_size) == (17, 300, 0.75)
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(api.SvoError):
            api.grid_clearance_default_params(g, bad)
    for field, value in (("na", 0), ("nb", 8193), ("cell_voxels", 0)):
        h = api.voxel_grid_default_params(0.1)
        setattr(h, field, value)
        with pytest.raises(api.SvoError):
            api.grid_clearance_default_params(h, 0.1)
    assert L.svo_grid_clearance_default_params(None, C.c_float(0.1), C.byref(d)) == -1
    assert L.svo_grid_clearance_default_params(C.byref(g), C.c_float(0.1), None) == -1
    assert api.grid_clearance_workspace_bytes(256, 256) == 4 * 256 * 256 and api.grid_clearance_workspace_bytes(1, 1) == 4
    assert api.grid_clearance_workspace_bytes(0, 5) == 0 and api.grid_clearance_workspace_bytes(5, -1) == 0
    assert api.grid_clearance_workspace_bytes(40000, 40000) == 4 * 40000 * 40000  # past 2^32
    # a null context is refused by both entries before anything else is looked at
    buf = (C.c_double * 12)()
    out = api.GridClearanceOut(C.addressof(buf))
    assert L.svo_grid_clearance_dev(None, buf, C.byref(d), buf, C.byref(out), None) == -1
    assert L.svo_grid_clearance(None, buf, C.byref(d), C.byref(out), None) == -1
    assert L.svo_grid_clearance_dev(None, None, None, None, None, None) == -1 and L.svo_grid_clearance(None, None, None, None, None) == -1


def test_grid_clearance_args_every_refusal_r2_the_sizes_and_the_defaults(tmp_path):
    """host/clearance_args.h on the CPU under ASan + UBSan: every refusal at its boundary with code and exact message, the order of
    the refusals, R2 at integer squares, just below them, at the clamp and where the quotient or the square overflows, the defaults,
    the workspace size past 2^32 and the launch geometry without 32-bit wrap."""
    _run_sanitized(tmp_path, "grid_clearance_args_test", "grid clearance args ok")


# ===================================================================================================== GPU
_SENT = {"dist2": (np.int32, 0x5555AAAA), "nearest": (np.int32, 0x3333CCCC), "clearance": (np.int32, 0x77777777), "blocked": (np.uint8, 0xBB)}


def _run(ctx, cls, prm, how="dev", skip=(), counts=True, keep=None):
    """One clearance by the named entry, as a G.Clearance (None for an output in `skip`, and for counts when they are left out).  The
    device entry runs into a dirty workspace and sentinel-filled outputs, one guard element before and behind each.  keep: a dict
    that receives the raw bytes of the workspace and of every output."""
    import torch
    p = _api_params(prm)
    if how == "host":
        *arrays, c = ctx.grid_clearance_host(cls, p)
        return G.Clearance(*arrays, tuple(c[k] for k in ("n_sources", "n_reached", "n_unreached", "n_blocked")))
    n = prm.na * prm.nb
    d_cls = torch.full((n + 2,), 2, dtype=torch.uint8, device="cuda")  # the guards would be sources
    d_cls[1:-1] = torch.from_numpy(np.array(cls).ravel()).cuda()
    ws = torch.full((n + 2,), 0x7F7F7F7F, dtype=torch.int32, device="cuda")
    bufs = {k: torch.full((n + 2,), v, dtype=getattr(torch, np.dtype(t).name), device="cuda") for k, (t, v) in _SENT.items()}
    cnt = torch.full((6,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ptr = {k: None if k in skip else b.data_ptr() + b.element_size() for k, b in bufs.items()}
    out = ctx.grid_clearance(d_cls.data_ptr() + 1, p, workspace_ptr=ws.data_ptr() + 4, counts_ptr=cnt.data_ptr() + 8 if counts else None,
                             **{k + "_ptr": v for k, v in ptr.items()})
    assert out["dist2"] == ptr["dist2"] and (out["na"], out["nb"]) == (prm.na, prm.nb)
    ctx.sync()  # the tensors go out of scope behind the return
    w = ws.cpu().numpy()
    assert w[0] == w[-1] == 0x7F7F7F7F
    assert np.array_equal(d_cls.cpu().numpy()[1:-1].reshape(cls.shape), cls)  # only read
    got = {}
    for k, (t, v) in _SENT.items():
        a = bufs[k].cpu().numpy()
        assert a[0] == v and a[-1] == v, k  # nothing beside the outputs is written
        if k in skip:
            assert (a == v).all(), k
            got[k] = None
        else:
            got[k] = a[1:-1].reshape(prm.na, prm.nb)
        if keep is not None:
            keep[k] = a.tobytes()
    if keep is not None:
        keep["workspace"] = w.tobytes()
    c = cnt.cpu().numpy()
    assert c[0] == c[-1] == -1 and (counts or (c == -1).all())
    # the workspace holds every row's nearest offset, or the word for none: a cell at offset 0 is a source
    assert np.array_equal(w[1:-1].reshape(cls.shape) == 0, got["dist2"].view(np.uint32) == 0)
    view = lambda a, t: None if a is None else a.view(t)
    return G.Clearance(view(got["dist2"], np.uint32), view(got["nearest"], np.uint32), view(got["clearance"], np.float32), got["blocked"],
                       tuple(int(v) for v in c[1:5]) if counts else None)


def _eq(got, w, what=""):
    for name in ("dist2", "nearest", "blocked"):
        if getattr(got, name) is not None:
            assert np.array_equal(getattr(got, name), getattr(w, name)), (what, name, int((getattr(got, name) != getattr(w, name)).sum()))
    if got.clearance is not None:
        assert np.array_equal(got.clearance.view(np.uint32), w.clearance.view(np.uint32)), (what, "clearance")
    if got.counts is not None:
        assert tuple(got.counts) == tuple(w.counts), (what, got.counts, w.counts)


@pytest.mark.gpu
@pytest.mark.parametrize("na,nb", G.SIZES)
def test_random_grids(ctx, na, nb):
    for density in G.DENSITIES:
        cls = G.random_grid(na, nb, density)
        for md in G.MAX_DISTS:
            w = want(na, nb, density, md)
            got = _run(ctx, cls, G.params(cls, md, inflate_radius=1.2))
            print(na, nb, density, md, "counts", got.counts)
            _eq(got, w, (density, md))


@pytest.mark.gpu
def test_constructed_grids(ctx):
    for name, (cls, prm, facts) in G.constructed().items():
        w = G.clearance_np(cls, prm)
        assert w.counts == facts["counts"], name
        for how in ("dev", "host"):
            _eq(_run(ctx, cls, prm, how), w, (name, how))


@pytest.mark.gpu
def test_every_byte_value_under_four_masks(ctx):
    cls, masks = G.all_values()
    for mask in masks:
        prm = G.params(cls, VALUES_MD, source_mask=mask, inflate_radius=0.6)
        w = G.clearance_np(cls, prm)
        assert w.counts[0] == bin(mask).count("1")
        for how in ("dev", "host"):
            _eq(_run(ctx, cls, prm, how), w, (hex(mask), how))


@pytest.mark.gpu
def test_inflation_at_a_square_just_below_it_at_zero_and_beyond_the_clamp(ctx):
    cls = _inflation_grid()
    for name, (radius, r2) in INFLATIONS.items():
        prm = G.params(cls, 5, inflate_radius=radius)
        w = G.clearance_np(cls, prm)
        assert G.r2_of(prm) == r2 and w.counts[3] == int(((w.dist2 > 0) & (w.dist2 <= r2)).sum()), name
        for how in ("dev", "host"):
            _eq(_run(ctx, cls, prm, how), w, (name, how))
    # another cell size: the clearance is the only output it moves
    prm = G.params(cls, 5, cell_size=0.3, inflate_radius=0.9)
    w = G.clearance_np(cls, prm)
    assert G.r2_of(prm) in (8, 9)
    _eq(_run(ctx, cls, prm), w, "0.3 per cell")


@pytest.mark.gpu
def test_optional_outputs_the_host_entry_and_a_repeated_call(ctx):
    from stereo_vo_amd import api
    na, nb, density, md = 65, 63, 0.05, 5
    cls = G.random_grid(na, nb, density)
    prm = G.params(cls, md, inflate_radius=1.2)
    w = want(na, nb, density, md)
    for skip in [(k,) for k in OUTPUTS] + [OUTPUTS]:
        got = _run(ctx, cls, prm, skip=skip)
        assert all(getattr(got, k) is None for k in skip) and got.dist2 is not None
        _eq(got, w, skip)
    _eq(_run(ctx, cls, prm, counts=False), w, "no counts")
    _eq(_run(ctx, cls, prm, skip=OUTPUTS, counts=False), w, "dist2 alone")
    # the host entry: everything, keywords instead of a parameter set, dist2 alone
    _eq(_run(ctx, cls, prm, "host"), w, "host")
    d2, near, clr, blk, c = ctx.grid_clearance_host(cls, max_dist=md, cell_size=0.5, inflate_radius=1.2)
    _eq(G.Clearance(d2, near, clr, blk, tuple(c.values())), w, "host by keywords")
    d2 = np.full((na, nb), 0x5555AAAA, np.uint32)
    p = _api_params(prm)
    assert ctx.L.svo_grid_clearance(ctx.h, cls.ctypes.data, C.byref(p), C.byref(api.GridClearanceOut(d2.ctypes.data)), None) == 0
    assert np.array_equal(d2, w.dist2)
    # twice: the same bytes in the workspace and in every output
    first, second = {}, {}
    _eq(_run(ctx, cls, prm, keep=first), w)
    _eq(_run(ctx, cls, prm, keep=second), w)
    assert first == second and set(first) == {"workspace", "dist2", "nearest", "clearance", "blocked"}


@pytest.mark.gpu
def test_bad_calls_launch_nothing_and_leave_the_context_usable(ctx):
    import torch
    from stereo_vo_amd import api
    L = ctx.L
    na, nb, density, md = 63, 65, 0.05, 5
    cls = G.random_grid(na, nb, density)
    good = G.params(cls, md, inflate_radius=1.2)
    n = na * nb
    d_cls = torch.from_numpy(np.array(cls).ravel()).cuda()
    ws = torch.full((n + 1,), 0x7F7F7F7F, dtype=torch.int32, device="cuda")
    u32 = torch.full((3, n + 1), 0x5555AAAA, dtype=torch.int32, device="cuda")
    u8 = torch.full((n,), 0xBB, dtype=torch.uint8, device="cuda")
    u64 = torch.full((5,), 0x6666666666666666, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    O = api.GridClearanceOut
    nan, inf = float("nan"), float("inf")
    d2p, nearp, clrp = (u32[k].data_ptr() for k in range(3))

    def dev(prm=good, cls_ptr=d_cls.data_ptr(), ws_ptr=ws.data_ptr(), out=None, counts=None, null_prm=False, null_out=False):
        o = out if out is not None else O(d2p, nearp, clrp, u8.data_ptr())
        p = _api_params(prm)
        return L.svo_grid_clearance_dev(ctx.h, cls_ptr, None if null_prm else C.byref(p), ws_ptr, None if null_out else C.byref(o), counts)

    r = good._replace
    host = np.full((na, nb), 0x5555AAAA, np.uint32)
    calls = [(lambda: dev(cls_ptr=None), "null cls"), (lambda: dev(null_prm=True), "null params"), (lambda: dev(ws_ptr=None), "null workspace"),
             (lambda: dev(null_out=True), "null out"), (lambda: dev(out=O(None, nearp)), "null dist2"),
             (lambda: dev(r(na=0)), "na outside"), (lambda: dev(r(na=8193)), "na outside"), (lambda: dev(r(nb=0)), "nb outside"),
             (lambda: dev(r(nb=8193)), "nb outside"), (lambda: dev(r(na=8192, nb=2049)), "na * nb"), (lambda: dev(r(source_mask=0)), "source_mask"),
             (lambda: dev(r(max_dist=0)), "max_dist"), (lambda: dev(r(max_dist=8192)), "max_dist"), (lambda: dev(r(cell_size=0.0)), "cell_size"),
             (lambda: dev(r(cell_size=-0.5)), "cell_size"), (lambda: dev(r(cell_size=nan)), "cell_size"), (lambda: dev(r(cell_size=inf)), "cell_size"),
             (lambda: dev(r(inflate_radius=-0.1)), "inflate_radius"), (lambda: dev(r(inflate_radius=nan)), "inflate_radius"),
             (lambda: dev(r(inflate_radius=inf)), "inflate_radius"),
             (lambda: dev(ws_ptr=ws.data_ptr() + 2), "workspace must be 4-byte"), (lambda: dev(out=O(d2p + 2)), "dist2 must be 4-byte"),
             (lambda: dev(out=O(d2p, nearp + 1)), "nearest must be 4-byte"), (lambda: dev(out=O(d2p, None, clrp + 2)), "clearance must be 4-byte"),
             (lambda: dev(counts=u64.data_ptr() + 4), "counts must be 8-byte"),
             (lambda: L.svo_grid_clearance(ctx.h, None, C.byref(_api_params(good)), C.byref(O(host.ctypes.data)), None), "null cls"),
             (lambda: L.svo_grid_clearance(ctx.h, cls.ctypes.data, None, C.byref(O(host.ctypes.data)), None), "null params"),
             (lambda: L.svo_grid_clearance(ctx.h, cls.ctypes.data, C.byref(_api_params(r(max_dist=0))), C.byref(O(host.ctypes.data)), None), "max_dist"),
             (lambda: L.svo_grid_clearance(ctx.h, cls.ctypes.data, C.byref(_api_params(good)), None, None), "null out"),
             (lambda: L.svo_grid_clearance(ctx.h, cls.ctypes.data, C.byref(_api_params(good)), C.byref(O(None)), None), "null dist2")]
    ctx.profile_select("grid_clearance")
    for call, word in calls:
        assert call() == -1 and word in L.svo_last_error(ctx.h).decode(), (word, L.svo_last_error(ctx.h).decode())
    assert ctx.profile_read()[1] == 0
    assert (u32.cpu().numpy() == 0x5555AAAA).all() and (u8.cpu().numpy() == 0xBB).all() and (u64.cpu().numpy() == 0x6666666666666666).all()
    assert (ws.cpu().numpy() == 0x7F7F7F7F).all() and (host == 0x5555AAAA).all()
    # the boundaries' accepted sides in one call: one cell, the largest max_dist, every mask bit, a huge radius
    assert dev(good._replace(na=1, nb=1, max_dist=8191, source_mask=0xFFFFFFFF, inflate_radius=1.7e308, cell_size=5e-324)) == 0
    assert ctx.profile_read()[1] == 1
    ctx.profile_select(None)
    with pytest.raises(api.SvoError):
        ctx.grid_clearance(d_cls.data_ptr(), _api_params(good), dist2_ptr=d2p)  # no workspace
    with pytest.raises(api.SvoError):
        ctx.grid_clearance_host(cls, max_dist=0, cell_size=0.5)
    with pytest.raises(ValueError):
        ctx.grid_clearance_host(cls, _api_params(good._replace(na=5)))
    # the context is what it was, and gives the clearance
    w = want(na, nb, density, md)
    _eq(_run(ctx, cls, good), w)
    _eq(_run(ctx, cls, good, "host"), w)
